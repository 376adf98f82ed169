// ivector-mean / ivector-subtract-global-mean / transform-vec / ivector-normalize-length - drop-in command lines for
// the vector tools the reference runs on the extracted embeddings (one executable, dispatching on its name):
//   ivector-mean <spk2utt-rspecifier> <ivector-rspecifier> <ivector-wspecifier> [<num-utt-wspecifier>]
//   ivector-mean <ivector-rspecifier> <mean-wxfilename>
//       egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:106-107, egs/sre/v2/run_sre10.sh:219-221,238
//   ivector-subtract-global-mean [<mean-rxfilename>] <ivector-rspecifier> <ivector-wspecifier>     run_sre10.sh:229,239,240
//   transform-vec <transform-rxfilename> <vec-rspecifier> <vec-wspecifier>                          run_sre10.sh:233,239,240
//   ivector-normalize-length [--normalize=true --scaleup=true] <ivector-rspecifier> <ivector-wspecifier>
// The arithmetic runs on the HIP device through libxvec_hip.so (backend.h); without a GPU the tools fail (exit 255).
// Semantics are upstream Kaldi's (not vendored in the reference, hence restated): speaker means accumulate in fp32 in
// spk2utt order, the global mean in fp64; log lines and exit codes follow the Kaldi idiom (0 iff something was written).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "backend.h"
#include "cli.h"
#include "kio.h"

namespace {

struct Args {
  std::vector<std::string> pos;   // set by main() for the tool that runs
  bool binary = true;          // --binary (ivector-mean's mean file)
  bool normalize = true;       // ivector-normalize-length
  bool scaleup = true;
  bool subtract_mean = true;   // ivector-subtract-global-mean
  int device = -1;
};

double Norm(const float* v, int n) {
  double s = 0;
  for (int i = 0; i < n; ++i) s += (double)v[i] * v[i];
  return sqrt(s);
}

constexpr int kBatch = 65536;   // vectors per device call of the streaming tools

int IvectorMean(const Args& a) {
  const int dev = xv::PickDevice(a.device);
  if (a.pos.size() == 2) {
    // global mean -> Kaldi vector object
    xv::SequentialVectorReader r(a.pos[0]);
    xv::Packed p;
    long n_err = 0;
    xv::ReadBatch(r, -1, &p, &n_err);
    if (p.n() == 0) throw xv::KioError("No iVectors read");
    std::vector<int32_t> off = {0, p.n()}, idx(p.n());
    for (int i = 0; i < p.n(); ++i) idx[i] = i;
    std::vector<float> mean(p.dim);
    xv::SegmentMean(dev, p.data.data(), p.n(), p.dim, off.data(), idx.data(), 1, /*acc64=*/true, mean.data());
    XLOG("Read " << p.n() << " iVectors.");
    xv::WriteVectorObject(a.pos[1], a.binary, mean.data(), p.dim);
    return 0;
  }
  if (a.pos.size() != 3 && a.pos.size() != 4) return xv::kUsageError;
  std::vector<xv::TokenList> spk2utt = xv::ReadTokenVectorTable(a.pos[0]);
  // the vector table is accessed by utterance key, as Kaldi's RandomAccessBaseFloatVectorReader
  xv::SequentialVectorReader r(a.pos[1]);
  xv::Packed p;
  long n_read_err = 0;
  xv::ReadBatch(r, -1, &p, &n_read_err);
  std::unordered_map<std::string, int> row;
  for (int i = 0; i < p.n(); ++i) row.emplace(p.keys[i], i);
  xv::TableWriter w(a.pos[2]);
  std::unique_ptr<xv::TableWriter> wn;
  if (a.pos.size() == 4) wn.reset(new xv::TableWriter(a.pos[3]));
  std::vector<int32_t> off = {0}, idx;
  std::vector<int> spk_of_seg;
  long num_spk_err = 0, num_utt_done = 0, num_utt_err = 0;
  for (size_t s = 0; s < spk2utt.size(); ++s) {
    const xv::TokenList& e = spk2utt[s];
    if (e.tokens.empty()) throw xv::KioError("Speaker with no utterances.");
    int count = 0;
    for (const std::string& utt : e.tokens) {
      auto it = row.find(utt);
      if (it == row.end()) {
        XWARN("No iVector present in input for utterance " << utt);
        ++num_utt_err;
      } else {
        idx.push_back(it->second);
        ++count;
        ++num_utt_done;
      }
    }
    if (count == 0) {
      XWARN("Not producing output for speaker " << e.key << " since no utterances had iVectors");
      ++num_spk_err;
    } else {
      off.push_back((int32_t)idx.size());
      spk_of_seg.push_back((int)s);
    }
  }
  const int n_seg = (int)spk_of_seg.size();
  std::vector<float> means((size_t)n_seg * (p.dim ? p.dim : 1));
  if (n_seg) xv::SegmentMean(dev, p.data.data(), p.n(), p.dim, off.data(), idx.data(), n_seg, /*acc64=*/false, means.data());
  std::vector<double> spk_sum(p.dim, 0.0);
  double spk_sumsq = 0;
  for (int g = 0; g < n_seg; ++g) {
    const float* m = means.data() + (size_t)g * p.dim;
    const std::string& spk = spk2utt[spk_of_seg[g]].key;
    w.WriteVec(spk, m, p.dim);
    if (wn) wn->WriteInt32(spk, off[g + 1] - off[g]);
    for (int k = 0; k < p.dim; ++k) {
      spk_sum[k] += m[k];
      spk_sumsq += (double)m[k] * m[k];
    }
  }
  w.Close();
  if (wn) wn->Close();
  XLOG("Computed mean of " << n_seg << " speakers (" << num_spk_err << " with no utterances), consisting of "
                           << num_utt_done << " utterances (" << num_utt_err << " absent from input).");
  if (n_seg != 0) {
    double mean_sq = 0;
    for (int k = 0; k < p.dim; ++k) mean_sq += (spk_sum[k] / n_seg) * (spk_sum[k] / n_seg);
    XLOG("Norm of mean of speakers is " << sqrt(mean_sq) << ", root-mean-square speaker-iVector length divided by sqrt(dim) is "
                                       << sqrt(spk_sumsq / ((double)n_seg * p.dim)));
  }
  return n_seg != 0 ? 0 : 1;
}

int SubtractGlobalMean(const Args& a) {
  const int dev = xv::PickDevice(a.device);
  if (a.pos.size() == 2) {
    // the mean of the input itself
    xv::SequentialVectorReader r(a.pos[0]);
    xv::Packed p;
    long n_err = 0;
    xv::ReadBatch(r, -1, &p, &n_err);
    XLOG("Read " << p.n() << " iVectors.");
    xv::TableWriter w(a.pos[1]);
    if (p.n() != 0) {
      std::vector<int32_t> off = {0, p.n()}, idx(p.n());
      for (int i = 0; i < p.n(); ++i) idx[i] = i;
      std::vector<float> mean(p.dim), out(p.data.size());
      xv::SegmentMean(dev, p.data.data(), p.n(), p.dim, off.data(), idx.data(), 1, true, mean.data());
      XLOG("Norm of iVector mean was " << Norm(mean.data(), p.dim));
      xv::BackendOptions o;
      o.mean = a.subtract_mean ? mean.data() : nullptr;
      xv::BackendApply(dev, p.data.data(), p.n(), p.dim, o, out.data(), nullptr);
      for (int i = 0; i < p.n(); ++i) w.WriteVec(p.keys[i], out.data() + (size_t)i * p.dim, p.dim);
    }
    w.Close();
    XLOG("Wrote " << p.n() << " mean-subtracted iVectors");
    return p.n() != 0 ? 0 : 1;
  }
  if (a.pos.size() != 3) return xv::kUsageError;
  std::vector<float> mean;
  xv::ReadVectorObject(a.pos[0], &mean);
  xv::SequentialVectorReader r(a.pos[1]);
  xv::TableWriter w(a.pos[2]);
  xv::Packed p;
  long n_err = 0, n_done = 0;
  std::vector<float> out;
  while (xv::ReadBatch(r, kBatch, &p, &n_err)) {
    if (p.dim != (int)mean.size())
      throw xv::KioError("iVector dimension " + std::to_string(p.dim) + " does not match the mean's " + std::to_string(mean.size()));
    out.resize(p.data.size());
    xv::BackendOptions o;
    o.mean = mean.data();
    xv::BackendApply(dev, p.data.data(), p.n(), p.dim, o, out.data(), nullptr);
    for (int i = 0; i < p.n(); ++i) w.WriteVec(p.keys[i], out.data() + (size_t)i * p.dim, p.dim);
    n_done += p.n();
  }
  w.Close();
  XLOG("Wrote " << n_done << " mean-subtracted iVectors");
  return n_done != 0 ? 0 : 1;
}

int TransformVec(const Args& a) {
  if (a.pos.size() != 3) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  xv::Matrix t;
  xv::ReadMatrixObject(a.pos[0], &t);
  xv::SequentialVectorReader r(a.pos[1]);
  xv::TableWriter w(a.pos[2]);
  xv::Packed p;
  long n_err = 0, n_done = 0;
  std::vector<float> out;
  while (xv::ReadBatch(r, kBatch, &p, &n_err)) {
    if (t.cols != p.dim && t.cols != p.dim + 1)
      throw xv::KioError("Dimension mismatch: input vector has dimension " + std::to_string(p.dim) + " and transform has " +
                         std::to_string(t.cols) + " columns.");
    out.resize((size_t)p.n() * t.rows);
    xv::BackendOptions o;
    o.transform = t.data.data();
    o.t_rows = t.rows;
    o.t_cols = t.cols;
    xv::BackendApply(dev, p.data.data(), p.n(), p.dim, o, out.data(), nullptr);
    for (int i = 0; i < p.n(); ++i) w.WriteVec(p.keys[i], out.data() + (size_t)i * t.rows, t.rows);
    n_done += p.n();
  }
  w.Close();
  XLOG("Applied transform to " << n_done << " vectors.");
  return n_done != 0 ? 0 : 1;
}

int NormalizeLength(const Args& a) {
  if (a.pos.size() != 2) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  xv::SequentialVectorReader r(a.pos[0]);
  xv::TableWriter w(a.pos[1]);
  xv::Packed p;
  long n_err = 0, n_done = 0;
  double tot_ratio = 0, tot_ratio2 = 0;
  std::vector<float> out, ratio;
  while (xv::ReadBatch(r, kBatch, &p, &n_err)) {
    out.resize(p.data.size());
    ratio.resize(p.n());
    xv::BackendOptions o;
    o.normalize = a.normalize;
    o.scaleup = a.scaleup;
    xv::BackendApply(dev, p.data.data(), p.n(), p.dim, o, out.data(), ratio.data());
    for (int i = 0; i < p.n(); ++i) {
      if (ratio[i] == 0.f) XWARN("Zero iVector");
      w.WriteVec(p.keys[i], out.data() + (size_t)i * p.dim, p.dim);
      tot_ratio += ratio[i];
      tot_ratio2 += (double)ratio[i] * ratio[i];
    }
    n_done += p.n();
  }
  w.Close();
  XLOG("Processed " << n_done << " iVectors.");
  if (n_done != 0) {
    const double avg = tot_ratio / n_done, var = tot_ratio2 / n_done - avg * avg;
    XLOG("Average ratio of iVector to expected length was " << avg << ", standard deviation was " << sqrt(var > 0 ? var : 0));
  }
  return n_done != 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  auto tool = [&](const char* name, const char* usage, int (*run)(const Args&)) {
    // All four tools know all of these, and count their arguments themselves.
    xv::CliTool t = {name, usage,
                     {xv::Bool("binary", &a.binary), xv::Bool("normalize", &a.normalize), xv::Bool("scaleup", &a.scaleup),
                      xv::Bool("subtract-mean", &a.subtract_mean), xv::LaxInt("device", &a.device)},
                     0, -1, [&a, run](const std::vector<std::string>& pos) { return a.pos = pos, run(a); }};
    t.underscores = false;
    t.bad_value_line = true;
    return t;
  };
  const std::vector<xv::CliTool> tools = {
      tool("ivector-mean",
           "With 3 or 4 arguments, averages iVectors over all the utterances of each speaker using the spk2utt file.\n"
           "With 2 arguments, averages all the iVectors of the input and writes the mean as a single vector.\n"
           "Usage: ivector-mean <spk2utt-rspecifier> <ivector-rspecifier> <ivector-wspecifier> [<num-utt-wspecifier>]\n"
           " or:   ivector-mean [--binary=true] <ivector-rspecifier> <mean-wxfilename>\n",
           IvectorMean),
      tool("ivector-subtract-global-mean",
           "Copies a table of iVectors but subtracts the global mean as it does so.  The mean may be specified as the first\n"
           "argument; if not, the sum of the input iVectors is used.\n"
           "Usage: ivector-subtract-global-mean [--subtract-mean=true] <ivector-rspecifier> <ivector-wspecifier>\n"
           " or:   ivector-subtract-global-mean <mean-rxfilename> <ivector-rspecifier> <ivector-wspecifier>\n",
           SubtractGlobalMean),
      tool("transform-vec",
           "This program applies a linear or affine transform to individual vectors, e.g. iVectors.\n"
           "Usage: transform-vec [options] <transform-rxfilename> <feats-rspecifier> <feats-wspecifier>\n",
           TransformVec),
      tool("ivector-normalize-length",
           "Normalize length of iVectors to equal sqrt(feature-dimension)\n"
           "Usage: ivector-normalize-length [--normalize=true] [--scaleup=true] <ivector-rspecifier> <ivector-wspecifier>\n",
           NormalizeLength),
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExact, "ivector-mean");
}
