// nnet-am-compute / nnet-am-info - drop-in command lines for the DNN i-vector path of egs/sre/v1
// (sid/init_full_ubm_from_dnn.sh:94-108, sid/train_ivector_extractor_dnn.sh:148-150, sid/extract_ivectors_dnn.sh:92-98).  One
// executable, dispatching on its exact base name:
//   nnet-am-compute [--apply-log=false --divide-by-priors=false --pad-input=true --chunk-size=0 --use-gpu=<any>] <model-in>
//                   <feature-rspecifier> <feature-or-loglikes-wspecifier>
//   nnet-am-info <model-in>
// Semantics: nnet2.h, nnet2_model.h.  nnet-am-compute runs on the device whatever --use-gpu says, and fails without a GPU (exit
// 255); nnet-am-info is host code and opens no device.  --chunk-size is checked (> 0 needs --pad-input=true) and changes no bit
// of the output: the device's own row blocks take its place.
#include <stdio.h>

#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "cli.h"
#include "kio.h"
#include "nnet2.h"
#include "stage_pipeline.h"

namespace {

struct ComputeOptions {
  bool apply_log = false, divide_by_priors = false, pad_input = true;
  int chunk_size = 0, device = -1;
  std::string use_gpu;
};

// the utterances of one device call
struct Batch {
  std::vector<std::string> keys;
  std::vector<int32_t> row_off = std::vector<int32_t>(1, 0);
  std::vector<float> feats, out;
};

constexpr int64_t kBatchRows = 8192;   // a batch is closed once it holds this many frames

int NnetAmCompute(const ComputeOptions& o, const std::vector<std::string>& pos) {
  if (o.chunk_size < 0) throw xv::KioError("--chunk-size=" + std::to_string(o.chunk_size) + " is out of range");
  if (o.chunk_size > 0 && !o.pad_input) throw xv::KioError("--chunk-size > 0 requires --pad-input=true");
  xv::Nnet2 net(pos[0]);
  const xv::Nnet2Dims& d = net.dims();
  const int flags = (o.apply_log ? xv::kNnet2ApplyLog : 0) | (o.divide_by_priors ? xv::kNnet2DivideByPriors : 0) | (o.pad_input ? xv::kNnet2PadInput : 0);
  net.CheckFlags(flags);
  const int dev = xv::PickDevice(o.device);
  xv::SequentialMatrixReader reader(pos[1]);
  xv::TableWriter writer(pos[2]);
  long num_done = 0, num_err = 0;
  int64_t frames = 0;
  bool ended = false, held = false;   // held: key / m are an utterance that did not fit the batch before
  std::string key, err;
  xv::Matrix m;
  // A batch is utterances of at most kBatchRows frames together, or ONE longer utterance: consume then hands that one's output
  // to the writer without a copy.
  const std::function<bool(Batch*)> produce = [&](Batch* b) {
    auto add = [&] {
      b->keys.push_back(key);
      b->feats.insert(b->feats.end(), m.Data(), m.Data() + (size_t)m.rows * m.cols);
      b->row_off.push_back(b->row_off.back() + m.rows);
      held = false;
    };
    if (held) add();
    while (!ended && b->row_off.back() < kBatchRows) {
      if (!reader.Next(&key, &m, &err)) {
        ended = true;
        break;
      }
      if (!err.empty()) {
        XWARN("Failed to read the features of " << key << ": " << err);
        ++num_err;
        continue;
      }
      if (m.cm) {
        xv::Matrix full;
        xv::ExpandCompressedView(m, &full);
        m = full;
      }
      if (m.rows == 0) {
        XWARN("Zero-length utterance: " << key);
        ++num_err;
        continue;
      }
      if (m.cols != d.input_dim) {
        XWARN("Dimension mismatch for utterance " << key << ": the features have " << m.cols << " columns, the model takes " << d.input_dim);
        ++num_err;
        continue;
      }
      if (net.OutRows(m.rows, flags) == 0) {
        XWARN("Utterance " << key << " has " << m.rows << " frames, fewer than the " << d.left_context + d.right_context + 1
                           << " the network's context needs without --pad-input: skipped");
        ++num_err;
        continue;
      }
      if (!b->keys.empty() && (int64_t)b->row_off.back() + m.rows > kBatchRows) {
        held = true;
        break;
      }
      add();
    }
    return !b->keys.empty();
  };
  const std::function<void(Batch*)> work = [&](Batch* b) {
    int64_t rows = 0;
    for (size_t u = 0; u < b->keys.size(); ++u) rows += net.OutRows(b->row_off[u + 1] - b->row_off[u], flags);
    b->out.resize((size_t)rows * d.output_dim);
    net.Compute(dev, b->feats.data(), b->row_off.data(), (int)b->keys.size(), flags, 0, b->out.data(), nullptr);
    std::vector<float>().swap(b->feats);
  };
  const std::function<void(Batch*)> consume = [&](Batch* b) {
    size_t at = 0;
    for (size_t u = 0; u < b->keys.size(); ++u) {
      xv::Matrix m;
      m.rows = (int)net.OutRows(b->row_off[u + 1] - b->row_off[u], flags);
      m.cols = d.output_dim;
      if (b->keys.size() == 1) m.data = std::move(b->out);
      else m.data.assign(b->out.begin() + at, b->out.begin() + at + (size_t)m.rows * m.cols);
      at += (size_t)m.rows * m.cols;
      writer.WriteMat(b->keys[u], m);
      frames += m.rows;
      ++num_done;
    }
  };
  xv::RunThreeStages<Batch>(produce, work, consume);
  writer.Close();
  XLOG("Done " << num_done << " utterances, " << frames << " frames; " << num_err << " with errors.");
  return num_done != 0 ? 0 : 1;
}

int NnetAmInfo(const std::string& rxfilename) {
  xv::Nnet2Model m;
  m.ReadFrom(rxfilename);
  fputs(m.Info().c_str(), stdout);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  ComputeOptions o;
  const std::vector<xv::CliTool> tools = {
      {"nnet-am-compute",
       "Does the neural net computation for each file of input features, and outputs as a matrix the result\n"
       "(the posteriors of the model's output layer; with --apply-log their logarithms).\n"
       "Usage: nnet-am-compute [options] <model-in> <feature-rspecifier> <feature-or-loglikes-wspecifier>\n"
       "Options: --apply-log (false) --divide-by-priors (false) --pad-input (true) --chunk-size (0: checked, without effect on the\n"
       "         output) --use-gpu (any value: the tool always runs on the device) --device=<gpu>\n",
       {xv::Bool("apply-log", &o.apply_log), xv::Bool("divide-by-priors", &o.divide_by_priors), xv::Bool("pad-input", &o.pad_input),
        xv::Int("chunk-size", &o.chunk_size), xv::String("use-gpu", &o.use_gpu), xv::Int("device", &o.device)},
       3, 3, [&](const Pos& pos) { return NnetAmCompute(o, pos); }},
      {"nnet-am-info",
       "Print human-readable information about the neural network acoustic model to the standard output\n"
       "Usage: nnet-am-info <nnet-in>\n"
       "e.g.: nnet-am-info 1.nnet\n",
       {}, 1, 1, [&](const Pos& pos) { return NnetAmInfo(pos[0]); }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExactOrRefuse);
}
