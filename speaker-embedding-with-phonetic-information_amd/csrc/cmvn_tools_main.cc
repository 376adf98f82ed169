// apply-cmvn-sliding / select-voiced-frames - drop-in command lines for stage 3 of the recipes (egs/sre/v2/run_sre10.sh:161-166
// through local/nnet3/xvector/prepare_feats_for_egs.sh:66-71; v3-v5: sid/nnet3_cvector/cvector/prepare_feats.sh:88-92 and
// :132-137); one executable, dispatching on its name:
//   apply-cmvn-sliding [--norm-vars=false --center --cmn-window --min-cmn-window] <feats-rspecifier> <feats-wspecifier>
//   select-voiced-frames <feats-rspecifier> <vad-rspecifier> <feats-wspecifier>
// apply-cmvn-sliding runs the device front-end's sliding-CMN kernels (compress.h CmvnSliding: the same launch path as the
// extractor's fused pipeline, fuse_pipe.h) and takes the options that pipeline recognises; without a GPU it fails (exit 255).
// select-voiced-frames is a row gather on the host and opens no device; its warnings are the fused front-end's
// (table_extract.cc), so that the two paths say the same.
#include <stdlib.h>

#include <string>
#include <vector>

#include "cli.h"
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

}  // namespace

int main(int argc, char** argv) {
  const bool select = xv::ProgramName(argv[0]).find("select") != std::string::npos;
  CmvnOptions o;
  xv::CliTool tool;
  tool.usage = select ? "Select a subset of frames of the input files, based on the output of\n"
                        "compute-vad or a similar program (a vector of length num-frames,\n"
                        "containing 1.0 for voiced, 0.0 for unvoiced).\n"
                        "Usage: select-voiced-frames [options] <feats-rspecifier> <vad-rspecifier> <feats-wspecifier>\n"
                      : "Apply sliding-window cepstral mean normalization per utterance.\n"
                        "Usage: apply-cmvn-sliding [options] <feats-rspecifier> <feats-wspecifier>\n"
                        "Options: --center (false) --cmn-window (600) --min-cmn-window (100) --norm-vars=false --device=<gpu>\n"
                        "Not built (refused): --norm-vars=true.\n";
  tool.config_file = false;
  tool.set = [&](const std::string& name, const std::string& val) {
    std::string n = name;
    for (char& c : n)
      if (c == '_') c = '-';
    if (n == "verbose" || n == "print-args" || n == "config") return xv::OptionResult::kOk;
    if (select) return xv::OptionResult::kUnknown;
    if (n == "norm-vars") {
      if (xv::ToBool(n, val)) throw xv::KioError("--norm-vars=true is not built: the device front-end subtracts the sliding mean only");
    } else if (n == "center") {
      o.center = xv::ToBool(n, val);
    } else if (n == "cmn-window") {
      o.cmn_window = xv::ToInt(n, val);
    } else if (n == "min-cmn-window") {
      o.min_cmn_window = xv::ToInt(n, val);
    } else if (n == "device") {
      o.device = atoi(val.c_str());
    } else {
      return xv::OptionResult::kUnknown;
    }
    return xv::OptionResult::kOk;
  };
  tool.run = [&](const std::vector<std::string>& pos) {
    if (pos.size() != (select ? 3u : 2u)) return xv::kUsageError;
    return select ? SelectVoicedFrames(pos) : ApplyCmvnSliding(o, pos);
  };
  return xv::CliMain(argc, argv, tool);
}
