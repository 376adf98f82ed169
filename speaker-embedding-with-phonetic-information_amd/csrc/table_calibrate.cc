// The arithmetic of a table job: the calibration sample, the measurement's log line and the shared choice.  See
// table_calibrate.h and table_extract.h.
#include "table_calibrate.h"

#include <chrono>
#include <memory>
#include <sstream>

#include "vad_verdict.h"

namespace xv {

Engine::Calibration CalibrateOnUtterances(Engine* engine, const ExtractOptions& opt, const std::vector<CalibUtt>& utts,
                                          const LogFn& log) {
  Engine::Calibration c;
  c.chosen = engine->fast_mode();
  if (!engine->can_switch_fast_mode()) return c;
  const int D = engine->info().input_dim;
  std::unique_ptr<RandomAccessVectorReader> vad;
  if (!opt.vad_rspecifier.empty()) vad.reset(new RandomAccessVectorReader(opt.vad_rspecifier));
  const bool use_frontend = opt.cmn_window > 0 || vad;
  std::vector<float> feats;
  std::vector<int32_t> offs(1, 0);
  for (size_t i = 0; i < utts.size() && (int)i < opt.calibrate_utts; ++i) {   // the first calibrate_utts utterances of the list, whoever calls
    const CalibUtt& u = utts[i];
    if (u.rows <= 0 || u.cols != D) continue;
    std::vector<float> tmp;
    const float* rows = u.data;
    int T = u.rows;
    if (use_frontend) {
      const std::vector<float>* v = nullptr;
      if (vad) {
        const VadVerdict verdict = JudgeVad(vad.get(), *u.key, T);
        if (!verdict.ok()) continue;   // the job will skip it as well, and say so
        v = verdict.decisions;
      }
      std::vector<int32_t> sel_row, sel_utt, raw_off = {0, T};
      for (int t = 0; t < T; ++t)
        if (!v || (*v)[t] != 0.f) {
          sel_row.push_back(t);
          sel_utt.push_back(0);
        }
      if (sel_row.empty()) continue;
      tmp.resize(sel_row.size() * (size_t)D);
      engine->FrontEndHost(u.data, raw_off.data(), 1, sel_row.data(), sel_utt.data(), (int)sel_row.size(), opt.cmn_window,
                           opt.cmn_center, opt.cmn_min_window, tmp.data());
      rows = tmp.data();
      T = (int)sel_row.size();
    }
    const int len = (opt.chunk_size > 0 && T > opt.chunk_size) ? opt.chunk_size : T;   // the utterance's first chunk
    if (len < engine->info().min_frames || (long)offs.back() + len > opt.max_batch_rows) continue;
    feats.insert(feats.end(), rows, rows + (size_t)len * D);
    offs.push_back(offs.back() + len);
  }
  const int n = (int)offs.size() - 1;
  const auto t_cal = std::chrono::steady_clock::now();
  // A measurement that fails - a device fault in a candidate arithmetic, a stream-K time-out, a device that does not reproduce
  // its own bits (Engine::Calibrate checks) - is REPEATED ONCE, with a WARNING that says why: the first forward passes of a
  // job's context are where four co-tenant jobs of a recipe meet on one GPU (GPUTEST r05, profiles/r06_cotenancy.md), and a
  // job of an hour should not die of - nor silently take another arithmetic from - one odd pass of its start-up measurement.
  // The second failure ends the job with its message.  (Errors of the EXTRACTION are never retried: a result is a result.)
  if (n > 0) {
    try {
      c = engine->Calibrate(feats.data(), offs.data(), n, opt.calibrate_tol);
    } catch (const EngineError& ex) {
      log("WARNING", std::string("calibration attempt failed (") + ex.what() + "); the measurement is repeated once");
      c = engine->Calibrate(feats.data(), offs.data(), n, opt.calibrate_tol);
    }
  }
  if (getenv("XVEC_TIMING")) {
    std::ostringstream t;
    t << "calibration: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t_cal).count() << " s for " << n << " chunks";
    log("LOG", t.str());
  }
  std::ostringstream m;
  m.precision(3);
  if (c.checked == 0) {
    m << "calibration: none of the " << utts.size() << " sampled utterances has a chunk long enough for the fast arithmetic; keeping "
      << PrecisionName(c.chosen);
  } else {
    m << "calibration on " << c.checked << " chunks against the three-pass arithmetic: fp16mx " << c.err_mx << " (on the " << c.checked_mx
      << " chunks it runs fast; it takes " << Engine::kCalibMinChunks << " to choose it), fp16mx2 " << c.err_mx2 << " (tolerance "
      << opt.calibrate_tol << ") -> " << PrecisionName(c.chosen);
    if (c.lite_mask) {
      m << " with " << __builtin_popcountll(c.lite_mask) << " of its layers in 1.25 passes (";
      bool first = true;
      for (size_t i = 0; i < engine->info().layers.size() && i < 64; ++i)
        if ((c.lite_mask >> i) & 1) {
          m << (first ? "" : ", ") << engine->info().layers[i].name;
          first = false;
        }
      m << ": " << c.err_lite << "; chosen on one half of the sample, " << c.err_holdout << " on the " << c.checked_holdout
        << " held-out chunks)";
    }
    if (c.lite_dropped) m << "; " << c.lite_dropped << " layer(s) admitted by the selection half failed the held-out half and were taken out again";
    if (c.tail > 0.f) m << "; projected tail of what runs (mean + 6 sd of the per-chunk error) " << c.tail;
    if (c.chosen != kPrecFp16Mx && c.err_mx <= opt.calibrate_tol && c.checked_mx >= Engine::kCalibMinChunks)
      m << "; fp16mx was within the tolerance on every sampled chunk but projects a tail of " << c.tail_mx << " and was turned down";
  }
  log("LOG", m.str());
  return c;
}

// Calibration sample of a table.  Tables whose objects can be addressed (an archive in a regular file, a script file) are
// indexed once - headers only - and calibrate_utts utterances are drawn EVENLY over the whole list: the reference's lists are
// sorted by speaker (utils/data/split_data.sh:18-21 splits them per speaker), so the head of a list is one or two speakers,
// and the choice governs every utterance of the job.  Streams (the feature pipe of extract_xvectors_new.sh:79) can only be
// read front to back: their sample is the head, and the log says so.  *strided tells which one it was.
static void SampleTable(const ExtractOptions& opt, const std::string& feat_rspec, std::vector<std::string>* keys,
                        std::vector<Matrix>* mats, bool* strided, long* n_list, TableIndex* index) {
  *strided = false;
  *n_list = -1;
  const int want = std::max(1, opt.calibrate_utts);
  {
    MatrixTableIndexer ix(feat_rspec);
    if (ix.usable()) {
      // ONE index of the table serves the sample and, through `index`, the batching pass of the extraction (the
      // headers of a 1 M-line scp were visited twice).  An object the indexer cannot get past (a text object, a truncated
      // archive) ends the index there and is remembered: the sample comes from what was indexed, and the extraction writes
      // everything in front of the bad object before it reports it - like the sequential reader and like the reference.
      TableIndex local;
      TableIndex& all = index ? *index : local;
      try {
        MatrixTableIndexer::Entry e;
        while (ix.Next(&e)) all.entries.push_back(std::move(e));
      } catch (const std::exception& ex) {
        all.error = ex.what();
      }
      all.valid = true;
      std::vector<size_t> good;
      for (size_t i = 0; i < all.entries.size(); ++i)
        if (all.entries[i].error.empty()) good.push_back(i);
      *strided = true;
      *n_list = (long)good.size();
      const long n = (long)good.size();
      ArchiveCursor cursor;
      long prev = -1;
      for (int i = 0; i < want && n > 0; ++i) {
        // centres of `want` equal slices of the list (all of it when it is shorter)
        const long k = n <= want ? i : (long)(((2 * (long long)i + 1) * n) / (2LL * want));
        if (k >= n || k == prev) continue;
        prev = k;
        Matrix m;
        try {
          ReadIndexedMatrix(all.entries[good[k]], &cursor, &m);
        } catch (const std::exception&) {
          continue;   // the extraction itself will report it
        }
        keys->push_back(all.entries[good[k]].key);
        mats->push_back(std::move(m));
      }
      return;
    }
  }
  SequentialMatrixReader rd(feat_rspec);
  std::string key, e;
  Matrix m;
  while ((int)keys->size() < want && rd.Next(&key, &m, &e)) {
    if (!e.empty()) continue;
    keys->push_back(key);
    mats->push_back(std::move(m));
  }
  // (the reader is closed here; for a pipe that ends the producer early, which is what a "head" of the list wants)
}

Engine::Calibration CalibrateOnTable(Engine* engine, const ExtractOptions& opt, const std::string& feat_rspec, const LogFn& log,
                                     TableIndex* index) {
  std::vector<std::string> keys;
  std::vector<Matrix> mats;
  bool strided = false;
  long n_list = -1;
  SampleTable(opt, feat_rspec, &keys, &mats, &strided, &n_list, index);
  std::ostringstream m;
  if (strided) m << "calibration sample: " << keys.size() << " utterances spread evenly over the " << n_list << " of the table";
  else m << "calibration sample: the first " << keys.size() << " utterances of the stream (a stream cannot be sampled any other way)";
  log("LOG", m.str());
  std::vector<CalibUtt> utts;
  for (size_t i = 0; i < keys.size(); ++i) utts.push_back(CalibUtt{&keys[i], mats[i].data.data(), mats[i].rows, mats[i].cols});
  return CalibrateOnUtterances(engine, opt, utts, log);
}

ArithmeticChoice::ArithmeticChoice(const std::vector<Engine*>& engines, const ExtractOptions& opt, const LogFn& log, const BatchSource::WarnFn& warn)
    : engines_(engines),
      engine_(engines[0]),
      opt_(opt),
      log_(log),
      warn_(warn),
      shared_(!opt.calibration_file.empty() && engine_->can_switch_fast_mode()) {}

void ArithmeticChoice::ShareChoice() {
  for (size_t k = 1; k < engines_.size(); ++k) {
    if (!engines_[k]->can_switch_fast_mode()) continue;
    engines_[k]->SetFastMode(engine_->fast_mode());
    if (engine_->lite_mask()) engines_[k]->SetLiteMask(engine_->lite_mask());
  }
}

void ArithmeticChoice::Adopt(const SharedChoice& sc, const std::string& how) {
  AdoptSharedChoice(engine_, sc, opt_.calibration_file);
  ShareChoice();
  std::ostringstream m;
  m << "arithmetic " << PrecisionName(sc.precision);
  if (sc.lite_mask) m << " with " << __builtin_popcountll(sc.lite_mask) << " of its layers in 1.25 passes (mask 0x" << std::hex << sc.lite_mask << std::dec << ")";
  m << ": " << how << " " << opt_.calibration_file << (sc.note.empty() ? "" : " [" + sc.note + "]");
  log_("LOG", m.str());
}

void ArithmeticChoice::Publish(const Engine::Calibration* c, const std::string& sample) {
  if (!shared_) return;
  SharedChoice mine, got;
  mine.model = engine_->info().fingerprint;
  mine.precision = engine_->fast_mode();
  mine.lite_mask = engine_->lite_mask();
  mine.tolerance = opt_.calibrate_tol;
  std::ostringstream n;
  n.precision(3);
  if (c && c->checked > 0)
    n << "measured on " << c->checked << " chunks (" << sample << "): fp16mx " << c->err_mx << ", fp16mx2 " << c->err_mx2 << ", projected tail "
      << c->tail;
  else
    n << "nothing could be measured (" << sample << "): the packed arithmetic";
  mine.note = n.str();
  const bool won = PublishCalibrationFile(opt_.calibration_file, mine, &got);
  Adopt(got, won ? "measured here and published as" : "another job published first; adopted from");
}

void ArithmeticChoice::ReadFromFile() {
  pending_ = opt_.calibrate && engine_->can_switch_fast_mode();
  if (shared_) {
    SharedChoice sc;
    pending_ = !ReadCalibrationFile(opt_.calibration_file, &sc);
    if (!pending_) Adopt(sc, "read from");
  }
  if (pending_ && !shared_)
    log_("LOG", "the arithmetic is measured for THIS job only (--calibrate without a --calibration file): jobs over other shards "
                "of the same list measure their own samples and may choose differently");
}

void ArithmeticChoice::MeasureOnTable(const std::string& feat_rspec, TableIndex* index) {
  pending_ = false;
  try {
    const Engine::Calibration c = CalibrateOnTable(engine_, opt_, feat_rspec, log_, index);
    ShareChoice();
    Publish(&c, "spread evenly over the table");
  } catch (const KioError& ex) {   // only the sample's own input errors are survivable
    warn_(std::string("calibration sample unreadable (") + ex.what() + "); keeping " + PrecisionName(engine_->fast_mode()));
    ShareChoice();
    Publish(nullptr, "sample unreadable");
  }
}

std::deque<Batch> ArithmeticChoice::MeasureOnStreamHead(Batch&& b, FirstError* fatal) {
  const bool last = b.last;
  held_utts_ += b.utts.size();
  held_.push_back(std::move(b));
  if (held_utts_ < (size_t)opt_.calibrate_utts && !last) return std::deque<Batch>();
  pending_ = false;
  if (!fatal->is_set()) {
    try {
      std::vector<CalibUtt> cu;
      for (const Batch& hb : held_)
        for (const Utt& u : hb.utts) cu.push_back(CalibUtt{&u.key, u.feats.Data(), u.feats.rows, u.feats.cols});
      if (!cu.empty()) {
        log_("LOG", "calibration sample: the first " + std::to_string(std::min(cu.size(), (size_t)opt_.calibrate_utts)) +
                        " utterances of the stream (a stream cannot be sampled any other way)");
        const Engine::Calibration c = CalibrateOnUtterances(engine_, opt_, cu, log_);
        ShareChoice();
        Publish(&c, "the head of a stream");
      } else {
        Publish(nullptr, "empty stream");
      }
    } catch (const std::exception& ex) {
      fatal->Set(ex.what());
    }
  }
  return std::move(held_);
}

}  // namespace xv
