// nnet3-compute's table loop: three stages (stage_pipeline.h) and the reader of a fused feature pipeline.  See table_extract.h.
#include "table_extract.h"

#include <math.h>
#include <string.h>

#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <unordered_map>
#include <vector>

#include "cmvn.h"
#include "feat_batch.h"
#include "kio.h"
#include "stage_pipeline.h"
#include "vad_verdict.h"

namespace xv {

namespace {

// One batch of nnet3-compute on its way through the three stages (stage_pipeline.h).
struct ComputeBatch {
  std::vector<std::string> keys;
  std::vector<int32_t> offs;     // [keys.size() + 1] rows that reach the network
  std::vector<float> feats;      // those rows - or, fused, the raw float rows the device front-end reads
  // fused pipelines only
  bool compressed = false;       // the raw rows are stored "CM" objects (cm / cm_off) instead of feats
  std::vector<int32_t> raw_off, sel_row, sel_utt, utt_norm;
  std::vector<uint8_t> cm;
  std::vector<int64_t> cm_off;
  int max_rows = 0;
  std::vector<float> norms;      // per-speaker pipeline: [n_norms][2][D]
  std::vector<float> out;        // written by the device stage; at least offs.back() * output_dim floats
  // Empty, with the memory it had: batches go round (RunTableCompute), since a fresh 100 MB buffer per batch costs more in
  // page faults than the stages hide.  `out` keeps its size too - nothing reads it before the device stage has written it.
  void Reset() {
    keys.clear();
    offs.clear();
    feats.clear();
    compressed = false;
    raw_off.clear();
    sel_row.clear();
    sel_utt.clear();
    utt_norm.clear();
    cm.clear();
    cm_off.clear();
    max_rows = 0;
    norms.clear();
  }
};

// The compressed objects of a batch as float rows: a table that mixes stored kinds does not close a batch early (the batches
// are those of the job run as commands), so the rare batch that meets both goes up as floats.
void ExpandOnHost(ComputeBatch* b, int D) {
  if (!b->compressed) return;
  b->feats.clear();
  for (size_t u = 0; u < b->cm_off.size(); ++u) {
    Matrix view, full;
    view.rows = b->raw_off[u + 1] - b->raw_off[u];
    view.cols = D;
    view.cm = b->cm.data() + b->cm_off[u];
    view.cm_bytes = (u + 1 < b->cm_off.size() ? (size_t)b->cm_off[u + 1] : b->cm.size()) - (size_t)b->cm_off[u];
    ExpandCompressedView(view, &full);
    b->feats.insert(b->feats.end(), full.data.begin(), full.data.end());
  }
  b->cm.clear();
  b->cm_off.clear();
  b->compressed = false;
}

// The reader stage of a fused job: the inner feature table joined with the side tables of the tools the job replaces, which
// it speaks for - their warnings, their counts, their closing lines.
class FusedComputeReader {
 public:
  FusedComputeReader(const ComputeFrontEnd& fe, int D, int max_batch_rows, const LogFn& log, TableExtractResult* res)
      : fe_(fe), D_(D), max_batch_rows_(max_batch_rows), log_(log), res_(res), feats_(fe.feats_rspecifier, 1, true) {
    if (!fe.vad_rspecifier.empty()) vad_.reset(new RandomAccessVectorReader(fe.vad_rspecifier));
    if (fe.kind != ComputeFrontEnd::kPerSpeaker) return;
    if (!fe.utt2spk_rspecifier.empty()) utt2spk_ = ReadTokenTable(fe.utt2spk_rspecifier);
    if (fe.stats_is_table) {
      stats_.reset(new RandomAccessDoubleMatrixReader(fe.stats_rxfilename));
    } else {
      Input in;
      in.Open(fe.stats_rxfilename);
      const bool binary = ReadBinaryHeader(in);
      ReadMatrixDouble(in, binary, &global_.rows, &global_.cols, &global_.data);
    }
  }

  // false: the table has ended and *b is empty
  bool Next(ComputeBatch* b) {
    b->offs.assign(1, 0);
    b->raw_off.assign(1, 0);
    std::map<std::string, int> norm_of;   // statistics key -> its norm in this batch
    FeatBatchReader::Batch one;
    std::vector<FeatBatchReader::Problem> problems;
    while (!done_) {
      problems.clear();
      const bool more = feats_.Next(&one, &problems);
      for (const auto& p : problems) {
        log_("WARNING", p.what.empty() ? "Empty feature matrix for utterance " + p.key : "Failed to read features for key " + p.key + ": " + p.what);
        ++norm_err_;
      }
      if (!more) {
        done_ = true;
        break;
      }
      const std::string& key = one.keys[0];
      const int rows = one.row_off[1], cols = one.cols;
      int norm = -1;
      if (fe_.kind == ComputeFrontEnd::kPerSpeaker && !FindNorm(key, cols, b, &norm_of, &norm)) continue;
      ++norm_done_;
      // select-voiced-frames
      const std::vector<float>* v = nullptr;
      int kept = rows;
      if (vad_) {
        const VadVerdict verdict = JudgeVad(vad_.get(), key, rows);
        if (!verdict.ok()) {
          log_("WARNING", verdict.Warning(key, rows));
          ++select_err_;
          if (verdict.kind != VadVerdict::kNoEntry) vad_->Forget(key);
          continue;
        }
        v = verdict.decisions;
        kept = verdict.kept;
        ++select_done_;
      }
      // nnet3-compute's own check, on what the pipeline would have handed it
      if (cols != D_) {
        std::ostringstream m;
        m << "feature dimension " << cols << " of utterance " << key << " does not match the model's " << D_;
        log_("WARNING", m.str());
        ++res_->num_fail;
        if (vad_) vad_->Forget(key);
        continue;
      }
      const int u = (int)b->keys.size();
      if (u > 0 && one.compressed != b->compressed) ExpandOnHost(b, D_);
      if (one.compressed && (u == 0 || b->compressed)) {
        b->compressed = true;
        b->cm_off.push_back((int64_t)b->cm.size());
        b->cm.insert(b->cm.end(), one.cm.begin(), one.cm.end());
      } else if (one.compressed) {
        ComputeBatch tmp;
        tmp.compressed = true;
        tmp.raw_off = {0, rows};
        tmp.cm_off = {0};
        tmp.cm = one.cm;
        ExpandOnHost(&tmp, D_);
        b->feats.insert(b->feats.end(), tmp.feats.begin(), tmp.feats.end());
      } else {
        b->feats.insert(b->feats.end(), one.feats.begin(), one.feats.end());
      }
      const int32_t r0 = b->raw_off.back();
      for (int t = 0; t < rows; ++t)
        if (!v || (*v)[t] != 0.f) {
          b->sel_row.push_back(r0 + t);
          b->sel_utt.push_back(u);
        }
      if (vad_) vad_->Forget(key);
      b->keys.push_back(key);
      b->raw_off.push_back(r0 + rows);
      b->offs.push_back(b->offs.back() + kept);
      b->utt_norm.push_back(norm);
      b->max_rows = std::max(b->max_rows, rows);
      if (b->offs.back() >= max_batch_rows_) break;
    }
    return !b->keys.empty();
  }

  // the closing lines of the tools the job stood in for
  void Report() const {
    std::ostringstream m;
    if (fe_.kind == ComputeFrontEnd::kPerSpeaker)
      m << "Applied cepstral mean " << (fe_.norm_vars ? "and variance " : "") << "normalization to " << norm_done_ << " utterances, errors on " << norm_err_;
    else
      m << "Applied sliding-window cepstral mean normalization to " << norm_done_ << " utterances, " << norm_err_ << " had errors.";
    log_("LOG", m.str());
    if (!vad_) return;
    std::ostringstream s;
    s << "Done selecting voiced frames; processed " << select_done_ << " utterances, " << select_err_ << " had errors.";
    log_("LOG", s.str());
  }

 private:
  // apply-cmvn's part: the norm of the utterance's speaker as a row of the batch's table.  false: no statistics (warned and
  // counted).  Statistics that do not fit the features, or without frames, are fatal, as they are to the tool.
  bool FindNorm(const std::string& key, int cols, ComputeBatch* b, std::map<std::string, int>* norm_of, int* norm) {
    const bool per_key = fe_.stats_is_table;
    std::string skey = key;
    auto none = [&] {
      log_("WARNING", "No normalization statistics available for key " + key + ", producing no output for this utterance");
      ++norm_err_;
      return false;
    };
    if (per_key && !fe_.utt2spk_rspecifier.empty()) {
      auto it = utt2spk_.find(skey);
      if (it == utt2spk_.end()) return none();
      skey = it->second;
    }
    if (!per_key) skey.clear();
    if (per_key && !stats_->HasKey(skey)) return none();
    const DoubleMatrix& st = per_key ? stats_->Value(skey) : global_;
    if (st.rows != 2 || st.cols != cols + 1) {
      std::ostringstream m;
      m << "Dimension mismatch: cmvn stats have dimension " << st.rows << "x" << st.cols << ", feats have dimension " << cols
        << " (utterance " << key << ")";
      throw KioError(m.str());
    }
    const bool keep = !per_key || !fe_.utt2spk_rspecifier.empty();   // a speaker's norm is computed, and its flooring warned about, once
    auto seen = kept_norm_.find(skey);
    std::vector<float> fresh;
    const std::vector<float>* nv = nullptr;
    if (keep && seen != kept_norm_.end()) {
      nv = &seen->second;
    } else {
      fresh.resize(2 * (size_t)cols);
      const int floored = CmvnNorm(st.data.data(), cols, true, fe_.norm_vars, false, nullptr, 0, fresh.data());
      if (floored) {
        std::ostringstream m;
        m << "Flooring cepstral variance from a value below 1.0e-20 to 1.0e-20 in " << floored << " dimension(s) (statistics of "
          << (skey.empty() ? fe_.stats_rxfilename : skey) << ")";
        log_("WARNING", m.str());
      }
      nv = keep ? &kept_norm_.emplace(skey, fresh).first->second : &fresh;
    }
    if (cols != D_) return true;   // never reaches the device: the caller reports the width
    auto known = norm_of->find(skey);
    if (known == norm_of->end()) {
      known = norm_of->emplace(skey, (int)(b->norms.size() / (2 * (size_t)D_))).first;
      b->norms.insert(b->norms.end(), nv->begin(), nv->end());
    }
    *norm = known->second;
    return true;
  }

  const ComputeFrontEnd fe_;
  const int D_, max_batch_rows_;
  const LogFn log_;
  TableExtractResult* res_;
  FeatBatchReader feats_;
  std::unique_ptr<RandomAccessVectorReader> vad_;
  std::unordered_map<std::string, std::string> utt2spk_;
  std::unique_ptr<RandomAccessDoubleMatrixReader> stats_;
  DoubleMatrix global_;
  std::map<std::string, std::vector<float>> kept_norm_;
  bool done_ = false;
  long norm_done_ = 0, norm_err_ = 0, select_done_ = 0, select_err_ = 0;
};

}  // namespace

TableExtractResult RunTableCompute(Engine* engine, int max_batch_rows, bool apply_exp, const std::string& feat_rspec,
                                   const std::string& mat_wspec, const LogFn& log, const ComputeFrontEnd* front) {
  TableExtractResult res;
  if (!engine->frame_mode()) throw EngineError("nnet3-compute needs a frame-level output node (this one follows the pooling)");
  const int D = engine->info().input_dim, E = engine->info().output_dim;
  const bool fused = front && front->kind != ComputeFrontEnd::kNone;
  TableWriter writer(mat_wspec);
  std::unique_ptr<SequentialMatrixReader> rd;
  std::unique_ptr<FusedComputeReader> fused_rd;
  if (fused) fused_rd.reset(new FusedComputeReader(*front, D, max_batch_rows, log, &res));
  else rd.reset(new SequentialMatrixReader(feat_rspec));
  const auto t0 = std::chrono::steady_clock::now();
  // read-ahead: the next batch, packed as the device stage takes it.  A batch closes when the rows that reach the network
  // reach max_batch_rows - fused or not, so that both form the same batches from the same utterances.
  auto read_plain = [&](ComputeBatch* b) {
    b->offs.assign(1, 0);
    std::string key, e;
    Matrix m;
    while (rd->Next(&key, &m, &e)) {
      if (!e.empty()) {
        log("WARNING", "failed to read features for " + key + ": " + e);
        ++res.num_fail;
        continue;
      }
      if (m.rows == 0) {
        log("WARNING", "Zero-length utterance: " + key);
        ++res.num_fail;
        continue;
      }
      if (m.cols != D) {
        std::ostringstream s;
        s << "feature dimension " << m.cols << " of utterance " << key << " does not match the model's " << D;
        log("WARNING", s.str());
        ++res.num_fail;
        continue;
      }
      const size_t at = b->feats.size(), count = (size_t)m.rows * D;
      b->feats.resize(at + count);
      memcpy(b->feats.data() + at, m.Data(), count * 4);
      b->keys.push_back(key);
      b->offs.push_back(b->offs.back() + m.rows);
      if (b->offs.back() >= max_batch_rows) break;
    }
    return !b->keys.empty();
  };
  // the device stage: the only one that touches the engine
  auto forward = [&](ComputeBatch* b) {
    const int B = (int)b->keys.size();
    if (b->out.size() < (size_t)b->offs[B] * E) b->out.resize((size_t)b->offs[B] * E);
    if (!fused) {
      engine->ForwardHost(b->feats.data(), b->offs.data(), B, b->out.data());
      return;
    }
    Engine::FrontEndInput fi;
    fi.raw = b->compressed ? nullptr : b->feats.data();
    fi.raw_off = b->raw_off.data();
    fi.n_utts = B;
    fi.sel_row = b->sel_row.data();
    fi.sel_utt = b->sel_utt.data();
    fi.n_out = (int)b->sel_row.size();
    if (b->compressed) {
      fi.cm = b->cm.data();
      fi.cm_off = b->cm_off.data();
      fi.cm_bytes = b->cm.size();
      fi.max_rows = b->max_rows;
    }
    if (front->kind == ComputeFrontEnd::kPerSpeaker) {
      fi.norms = b->norms.data();
      fi.n_norms = (int)(b->norms.size() / (2 * (size_t)D));
      fi.utt_norm = b->utt_norm.data();
    } else {
      fi.cmn_window = front->cmn_window;
      fi.center = front->center;
      fi.min_window = front->min_window;
    }
    engine->ForwardFrontHost(fi, b->offs.data(), B, b->out.data());
  };
  // write-behind; --apply-exp stays on the host (glibc's expf and the device's differ in the last bit)
  auto write = [&](ComputeBatch* b) {
    for (size_t i = 0; i < b->keys.size(); ++i) {
      Matrix m;
      m.rows = b->offs[i + 1] - b->offs[i];
      m.cols = E;
      m.data.assign(b->out.begin() + (size_t)b->offs[i] * E, b->out.begin() + (size_t)b->offs[i + 1] * E);
      if (apply_exp)
        for (float& v : m.data) v = expf(v);
      writer.WriteMat(b->keys[i], m);
      res.frames += m.rows;
      ++res.num_success;
    }
  };
  // the batches the writer is done with go back to the reader
  std::mutex pool_mu;
  std::vector<ComputeBatch> pool;
  auto produce = [&](ComputeBatch* b) {
    {
      std::lock_guard<std::mutex> lk(pool_mu);
      if (!pool.empty()) {
        *b = std::move(pool.back());
        pool.pop_back();
      }
    }
    b->Reset();
    return fused ? fused_rd->Next(b) : read_plain(b);
  };
  auto consume = [&](ComputeBatch* b) {
    write(b);
    std::lock_guard<std::mutex> lk(pool_mu);
    pool.push_back(std::move(*b));
  };
  RunThreeStages<ComputeBatch>(produce, forward, consume, 2);
  if (fused) fused_rd->Report();
  else res.reader_status = rd->Close();
  writer.Close();
  res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return res;
}

}  // namespace xv
