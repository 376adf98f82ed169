// apply-cmvn-sliding / select-voiced-frames - drop-in command lines for stage 3 of the recipes (egs/sre/v2/run_sre10.sh:161-166
// through local/nnet3/xvector/prepare_feats_for_egs.sh:66-71; v3-v5: sid/nnet3_cvector/cvector/prepare_feats.sh:88-92 and
// :132-137) - and compute-cmvn-stats / apply-cmvn, the per-speaker normalisation in front of the acoustic-model path
// (steps/compute_cmvn_stats.sh:104; sid/nnet3_cvector/am/extract_bn.sh:59).  One executable, dispatching on its name:
//   apply-cmvn-sliding [--norm-vars=false --center --cmn-window --min-cmn-window] <feats-rspecifier> <feats-wspecifier>
//   select-voiced-frames <feats-rspecifier> <vad-rspecifier> <feats-wspecifier>
//   compute-cmvn-stats [--spk2utt=<rspecifier>] [--binary=true] <feats-rspecifier> (<stats-wspecifier>|<stats-wxfilename>)
//   apply-cmvn [--utt2spk=<rspecifier>] [--norm-means=true] [--norm-vars=false] [--skip-dims=a:b:c] [--reverse=false]
//              (<stats-rspecifier>|<stats-rxfilename>) <feats-rspecifier> <feats-wspecifier>
// compute-cmvn-stats sums on the device (cmvn.h: fp64, an order that depends on the matrix alone) and adds the utterances of a
// speaker on the host in spk2utt order; apply-cmvn computes the norms on the host and runs the affine map on the device.  Both
// read the features ahead in batches, stored "CM" objects going up as they are, and fail without a GPU (exit 255); only
// apply-cmvn --norm-means=false, which copies the features through, opens no device.
// apply-cmvn-sliding runs the device front-end's sliding-CMN kernels (compress.h CmvnSliding: the same launch path as the
// extractor's fused pipeline, fuse_pipe.h) and takes the options that pipeline recognises; without a GPU it fails (exit 255).
// select-voiced-frames is a row gather on the host and opens no device; its warnings are the fused front-end's
// (table_extract.cc), so that the two paths say the same.
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include <map>
#include <unordered_map>

#include "cli.h"
#include "cmvn.h"
#include "compress.h"
#include "kio.h"

namespace {

constexpr int64_t kBatchFloats = 16 << 20;   // feature values per device call

struct CmvnOptions {
  int cmn_window = 600, min_cmn_window = 100;   // Kaldi's SlidingWindowCmnOptions
  bool center = false;
  int device = -1;
};

int ApplyCmvnSliding(const CmvnOptions& o, const std::vector<std::string>& pos) {
  const int dev = xv::PickDevice(o.device);
  xv::SequentialMatrixReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_done = 0, num_err = 0;
  std::vector<std::string> keys;
  std::vector<float> feats, out;
  std::vector<int32_t> off = {0};
  int dim = 0;
  auto flush = [&] {
    if (keys.empty()) return;
    out.resize(feats.size());
    xv::CmvnSliding(dev, feats.data(), off.data(), (int)keys.size(), dim, o.cmn_window, o.min_cmn_window, o.center, out.data());
    for (size_t u = 0; u < keys.size(); ++u) {
      xv::Matrix m;
      m.rows = off[u + 1] - off[u];
      m.cols = dim;
      m.data.assign(out.begin() + (size_t)off[u] * dim, out.begin() + (size_t)off[u + 1] * dim);
      writer.WriteMat(keys[u], m);
      ++num_done;
    }
    keys.clear();
    feats.clear();
    off.assign(1, 0);
  };
  std::string key, err;
  xv::Matrix m;
  while (reader.Next(&key, &m, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read features for key " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (m.rows == 0) {
      XWARN("Empty feature matrix for utterance " << key);
      ++num_err;
      continue;
    }
    if (dim != 0 && m.cols != dim) flush();   // a table may mix dimensions; a batch may not
    dim = m.cols;
    keys.push_back(key);
    feats.insert(feats.end(), m.Data(), m.Data() + (size_t)m.rows * m.cols);
    off.push_back(off.back() + m.rows);
    if ((int64_t)feats.size() >= kBatchFloats) flush();
  }
  flush();
  writer.Close();
  XLOG("Applied sliding-window cepstral mean normalization to " << num_done << " utterances, " << num_err << " had errors.");
  return num_done != 0 ? 0 : 1;
}

int SelectVoicedFrames(const std::vector<std::string>& pos) {
  xv::SequentialMatrixReader reader(pos[0]);
  xv::RandomAccessVectorReader vad(pos[1]);
  xv::TableWriter writer(pos[2]);
  long num_done = 0, num_err = 0;
  std::string key, err;
  xv::Matrix m, voiced;
  while (reader.Next(&key, &m, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read features for key " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (m.rows == 0) {
      XWARN("Empty feature matrix for utterance " << key);
      ++num_err;
      continue;
    }
    if (!vad.HasKey(key)) {
      XWARN("No VAD input found for utterance " << key);
      ++num_err;
      continue;
    }
    const std::vector<float>& v = vad.Value(key);
    if ((int)v.size() != m.rows) {
      XWARN("Mismatch in number of frames " << m.rows << " for features and VAD " << v.size() << ", for utterance " << key);
      ++num_err;
      vad.Forget(key);
      continue;
    }
    voiced.cols = m.cols;
    voiced.data.clear();
    for (int r = 0; r < m.rows; ++r)
      if (v[r] != 0.f) voiced.data.insert(voiced.data.end(), m.Row(r), m.Row(r) + m.cols);
    voiced.rows = (int)(voiced.data.size() / (size_t)m.cols);
    vad.Forget(key);
    if (voiced.rows == 0) {
      XWARN("No features were judged as voiced for utterance " << key);
      ++num_err;
      continue;
    }
    writer.WriteMat(key, voiced);
    ++num_done;
  }
  writer.Close();
  XLOG("Done selecting voiced frames; processed " << num_done << " utterances, " << num_err << " had errors.");
  return num_done != 0 ? 0 : 1;
}


constexpr int64_t kBatchFrames = 1 << 18;   // frames read ahead per device call of the two per-speaker tools

struct StatsOptions {
  std::string spk2utt;
  bool binary = true;
  int device = -1;
};

int ComputeCmvnStats(const StatsOptions& o, const std::vector<std::string>& pos) {
  const int dev = xv::PickDevice(o.device);
  const bool table = xv::IsTable(pos[1]);
  if (!o.spk2utt.empty() && !table) throw xv::KioError("--spk2utt option not compatible with wxfilename as output (did you forget ark:?)");
  std::vector<xv::TokenList> spk2utt;
  if (!o.spk2utt.empty()) spk2utt = xv::ReadTokenVectorTable(o.spk2utt);
  std::unique_ptr<xv::TableWriter> writer;
  if (table) writer.reset(new xv::TableWriter(pos[1]));
  xv::FeatBatchWalk walk(pos[0], kBatchFrames, true, xv::FeatProblems::kCount);
  long num_done = 0;
  std::unordered_map<std::string, std::vector<double>> utt_stats;   // --spk2utt: looked up by key afterwards
  std::vector<double> global;
  std::vector<double> stats;
  long num_err = walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    const int n = (int)b.keys.size(), w = b.cols + 1;
    stats.assign((size_t)n * 2 * w, 0.0);
    const xv::CmvnCompressed cm = b.View();
    xv::CmvnStats(dev, b.feats.data(), b.row_off.data(), n, b.cols, stats.data(), nullptr, b.compressed ? &cm : nullptr);
    for (int u = 0; u < n; ++u) {
      const double* st = stats.data() + (size_t)u * 2 * w;
      if (!spk2utt.empty()) {
        utt_stats.emplace(b.keys[u], std::vector<double>(st, st + 2 * w));   // the first entry of a key wins
      } else if (table) {
        writer->WriteMatDouble(b.keys[u], st, 2, w);
        ++num_done;
      } else {
        if (global.empty()) global.assign(2 * (size_t)w, 0.0);
        if (global.size() != 2 * (size_t)w) throw xv::KioError("Dimension mismatch: utterance " + b.keys[u] + " has " + std::to_string(b.cols) + " columns");
        for (int i = 0; i < 2 * w; ++i) global[i] += st[i];
        ++num_done;
      }
    }
  });
  if (!spk2utt.empty()) {
    for (const xv::TokenList& spk : spk2utt) {
      std::vector<double> acc;
      for (const std::string& utt : spk.tokens) {
        auto it = utt_stats.find(utt);
        if (it == utt_stats.end()) {
          XWARN("Did not find features for utterance " << utt);
          ++num_err;
          continue;
        }
        if (acc.empty()) acc.assign(it->second.size(), 0.0);
        if (acc.size() != it->second.size()) throw xv::KioError("Dimension mismatch among the utterances of speaker " + spk.key);
        for (size_t i = 0; i < acc.size(); ++i) acc[i] += it->second[i];   // spk2utt list order, fp64
        ++num_done;
      }
      if (acc.empty()) {
        XWARN("No stats accumulated for speaker " << spk.key);
        continue;
      }
      writer->WriteMatDouble(spk.key, acc.data(), 2, (int)(acc.size() / 2));
    }
  } else if (!table && !global.empty()) {
    xv::Output out;
    out.Open(pos[1]);
    if (o.binary) out.Write("\0B", 2);
    xv::WriteMatrixDouble(out, o.binary, global.data(), 2, (int)(global.size() / 2));
    if (out.Close() != 0) throw xv::KioError("error closing output " + pos[1]);
    XLOG("Wrote global CMVN stats to " << pos[1]);
  }
  if (writer) writer->Close();
  XLOG("Done accumulating CMVN stats for " << num_done << " utterances; " << num_err << " had errors.");
  return num_done != 0 ? 0 : 1;
}

struct ApplyOptions {
  std::string utt2spk;
  bool norm_means = true, norm_vars = false, reverse = false;
  std::vector<int> skip_dims;
  int device = -1;
};

int ApplyCmvn(const ApplyOptions& o, const std::vector<std::string>& pos) {
  if (o.norm_vars && !o.norm_means) throw xv::KioError("You cannot normalize the variance but not the mean.");
  const bool per_key = xv::IsTable(pos[0]);
  std::unordered_map<std::string, std::string> utt2spk;
  if (!o.utt2spk.empty()) utt2spk = xv::ReadTokenTable(o.utt2spk);
  std::unique_ptr<xv::RandomAccessDoubleMatrixReader> table;
  xv::DoubleMatrix global;
  if (per_key) {
    table.reset(new xv::RandomAccessDoubleMatrixReader(pos[0]));
  } else {
    xv::Input in;
    in.Open(pos[0]);
    const bool binary = xv::ReadBinaryHeader(in);
    xv::ReadMatrixDouble(in, binary, &global.rows, &global.cols, &global.data);
  }
  const int dev = o.norm_means ? xv::PickDevice(o.device) : -1;
  xv::TableWriter writer(pos[2]);
  // --norm-means=false copies the features through: floats from the host readers, no device
  xv::FeatBatchWalk walk(pos[1], kBatchFrames, o.norm_means, xv::FeatProblems::kCount);
  long num_done = 0, num_err = 0;
  std::vector<float> norms, out;
  std::vector<int32_t> utt_norm;
  // A speaker's (or the global) norm is computed once, and its flooring warning given once, however many batches its utterances
  // are spread over.  Per-utterance statistics are met once each and are not kept.
  const bool keep = !per_key || !o.utt2spk.empty();
  std::map<std::string, std::vector<float>> kept_norm;
  const long unread = walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    const int n = (int)b.keys.size();
    norms.clear();
    utt_norm.assign(n, -1);
    std::map<std::string, int> norm_of;   // statistics key -> its norm in this batch
    for (int u = 0; u < n && o.norm_means; ++u) {
      std::string skey = b.keys[u];
      if (per_key && !o.utt2spk.empty()) {
        auto it = utt2spk.find(skey);
        if (it == utt2spk.end()) {   // a key the map does not have finds no statistics
          XWARN("No normalization statistics available for key " << b.keys[u] << ", producing no output for this utterance");
          ++num_err;
          continue;
        }
        skey = it->second;
      }
      if (!per_key) skey.clear();
      auto known = norm_of.find(skey);
      if (known != norm_of.end()) {
        utt_norm[u] = known->second;
        continue;
      }
      if (per_key && !table->HasKey(skey)) {
        XWARN("No normalization statistics available for key " << b.keys[u] << ", producing no output for this utterance");
        ++num_err;
        continue;
      }
      const xv::DoubleMatrix& st = per_key ? table->Value(skey) : global;
      if (st.rows != 2 || st.cols != b.cols + 1) {
        std::ostringstream m;
        m << "Dimension mismatch: cmvn stats have dimension " << st.rows << "x" << st.cols << ", feats have dimension " << b.cols
          << " (utterance " << b.keys[u] << ")";
        throw xv::KioError(m.str());
      }
      const int k = (int)(norms.size() / (2 * (size_t)b.cols));
      norms.resize(norms.size() + 2 * (size_t)b.cols);
      float* norm = norms.data() + (size_t)k * 2 * b.cols;
      auto seen = keep ? kept_norm.find(skey) : kept_norm.end();
      if (seen != kept_norm.end()) {   // same statistics, same column count (checked above): same norm
        std::copy(seen->second.begin(), seen->second.end(), norm);
      } else {
        const int floored = xv::CmvnNorm(st.data.data(), b.cols, o.norm_means, o.norm_vars, o.reverse, o.skip_dims.data(),
                                         (int)o.skip_dims.size(), norm);
        if (floored) XWARN("Flooring cepstral variance from a value below 1.0e-20 to 1.0e-20 in " << floored << " dimension(s) (statistics of " << (skey.empty() ? pos[0] : skey) << ")");
        if (keep) kept_norm.emplace(skey, std::vector<float>(norm, norm + 2 * (size_t)b.cols));
      }
      norm_of.emplace(skey, k);
      utt_norm[u] = k;
    }
    const float* result = b.feats.data();
    if (o.norm_means) {
      out.resize((size_t)b.row_off[n] * b.cols);
      const xv::CmvnCompressed cm = b.View();
      xv::CmvnApply(dev, b.feats.data(), b.row_off.data(), n, b.cols, norms.data(), (int)(norms.size() / (2 * (size_t)b.cols)),
                    utt_norm.data(), out.data(), nullptr, b.compressed ? &cm : nullptr);
      result = out.data();
    }
    for (int u = 0; u < n; ++u) {
      if (o.norm_means && utt_norm[u] < 0) continue;
      xv::Matrix m;
      m.rows = b.row_off[u + 1] - b.row_off[u];
      m.cols = b.cols;
      m.data.assign(result + (size_t)b.row_off[u] * b.cols, result + (size_t)b.row_off[u + 1] * b.cols);
      writer.WriteMat(b.keys[u], m);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Applied cepstral mean " << (o.norm_vars ? "and variance " : "") << "normalization to " << num_done << " utterances, errors on "
                                << unread + num_err);
  return num_done != 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  CmvnOptions o;
  StatsOptions so;
  ApplyOptions ao;
  const std::vector<xv::CliTool> tools = {
      {"select-voiced-frames",
       "Select a subset of frames of the input files, based on the output of\n"
       "compute-vad or a similar program (a vector of length num-frames,\n"
       "containing 1.0 for voiced, 0.0 for unvoiced).\n"
       "Usage: select-voiced-frames [options] <feats-rspecifier> <vad-rspecifier> <feats-wspecifier>\n",
       {}, 3, 3, [&](const Pos& pos) { return SelectVoicedFrames(pos); }, "select"},
      {"compute-cmvn-stats",
       "Compute cepstral mean and variance normalization statistics, per utterance or, with --spk2utt, per speaker;\n"
       "with a file instead of a table as the output, one global matrix.\n"
       "Usage: compute-cmvn-stats [options] <feats-rspecifier> (<stats-wspecifier>|<stats-wxfilename>)\n"
       "Options: --spk2utt=<rspecifier> --binary (true) --device=<gpu>\n"
       "Not built (refused): --weights.\n",
       {xv::String("spk2utt", &so.spk2utt), xv::Bool("binary", &so.binary), xv::Int("device", &so.device),
        xv::Refused("weights", "--weights is not built: no script of the recipes passes it")},
       2, 2, [&](const Pos& pos) { return ComputeCmvnStats(so, pos); }},
      {"apply-cmvn-sliding",
       "Apply sliding-window cepstral mean normalization per utterance.\n"
       "Usage: apply-cmvn-sliding [options] <feats-rspecifier> <feats-wspecifier>\n"
       "Options: --center (false) --cmn-window (600) --min-cmn-window (100) --norm-vars=false --device=<gpu>\n"
       "Not built (refused): --norm-vars=true.\n",
       {xv::RefusedIfTrue("norm-vars", "--norm-vars=true is not built: the device front-end subtracts the sliding mean only"),
        xv::Bool("center", &o.center), xv::Int("cmn-window", &o.cmn_window), xv::Int("min-cmn-window", &o.min_cmn_window),
        xv::LaxInt("device", &o.device)},
       2, 2, [&](const Pos& pos) { return ApplyCmvnSliding(o, pos); }, "sliding"},
      {"apply-cmvn",
       "Apply cepstral mean and (optionally) variance normalization, per utterance or per speaker (--utt2spk), or with\n"
       "one global statistics matrix.\n"
       "Usage: apply-cmvn [options] (<cmvn-stats-rspecifier>|<cmvn-stats-rxfilename>) <feats-rspecifier> <feats-wspecifier>\n"
       "Options: --utt2spk=<rspecifier> --norm-means (true) --norm-vars (false) --skip-dims=a:b:c --reverse (false) --device=<gpu>\n",
       {xv::String("utt2spk", &ao.utt2spk), xv::Bool("norm-means", &ao.norm_means), xv::Bool("norm-vars", &ao.norm_vars),
        xv::Bool("reverse", &ao.reverse), xv::Int("device", &ao.device), xv::Custom("skip-dims", [&](const std::string&, const std::string& val) {
          if (!xv::ParseSkipDims(val, &ao.skip_dims)) throw xv::KioError("Bad --skip-dims option (should be colon-separated list of integers)");
          return true;
        })},
       3, 3, [&](const Pos& pos) { return ApplyCmvn(ao, pos); }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kContains, "apply-cmvn-sliding");
}
