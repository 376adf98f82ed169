// The device side of the table loop.  See table_consumer.h.
#include "table_consumer.h"

#include <algorithm>
#include <chrono>
#include <sstream>

#include "backend.h"
#include "vad_verdict.h"

namespace xv {

namespace {
typedef std::chrono::steady_clock::time_point TimePoint;
TimePoint Now() { return std::chrono::steady_clock::now(); }
double Secs(TimePoint a, TimePoint b) { return std::chrono::duration<double>(b - a).count(); }
constexpr int NS = Engine::kNumHostSlots;
}  // namespace

Consumer::Consumer(Engine* engine, ConsumerShared* shared)
    : eng_(engine),
      s_(shared),
      D_(engine->info().input_dim),
      E_(engine->info().output_dim),
      use_frontend_(shared->opt.cmn_window > 0 || shared->vad),
      has_backend_(!shared->opt.backend_mean.empty() || !shared->opt.backend_transform.empty() || shared->opt.backend_normalize),
      work_(NS) {}

void Consumer::Run(BoundedQueue<std::pair<long, Batch>>* inbox) {
  std::pair<long, Batch> item;
  while (inbox->Pop(&item)) {
    try {
      Process(std::move(item.second), item.first);
    } catch (const std::exception& ex) {   // (Process catches what the extraction throws; this is for the unexpected)
      s_->fatal->Set(ex.what());
    }
  }
  Drain();
}

// THE place that keeps the writer's invariant for a batch that arrives: its number g is delivered here, empty, unless the batch
// was submitted - then it sits in a slot, and Finalize (from a later Process, or from Drain) delivers it.
void Consumer::Process(Batch&& b, long g) {
  bool submitted_batch = false;
  if (!b.utts.empty() && !s_->fatal->is_set()) {
    try {
      const TimePoint tp0 = Now();
      Work& w = work_[cur_];
      w.b = std::move(b);
      w.g = g;
      RejectWrongDimension(&w);
      bool submitted = use_frontend_ && !w.idx.empty() && SubmitFrontEnd(&w);
      if (s_->vad && use_frontend_) {
        // the VAD decisions of this batch have done their work (the selection tables are built, or the host path has run)
        std::lock_guard<std::mutex> vlk(s_->vad_mu);
        for (const Utt& u : w.b.utts) s_->vad->Forget(u.key);
      }
      const TimePoint tp1 = Now();
      t_pack += Secs(tp0, tp1);
      const int n = (int)w.idx.size();
      if (n) {
        if (!submitted) {
          if (use_frontend_) w.job.Start(eng_, s_->opt, cur_, seq_++, w.packed.data(), w.offs.data(), n);   // front-end result (host)
          else w.job.StartPtrs(eng_, s_->opt, cur_, seq_++, w.uptr.data(), w.urows.data(), n);
        }
        const TimePoint tp2 = Now();
        t_start += Secs(tp1, tp2);
        submitted_batch = true;
        cur_ = (cur_ + 1) % NS;
        Work& oldest = work_[cur_];   // the slot the next batch will use
        if (oldest.job.active()) Finalize(&oldest);
        t_fin += Secs(tp2, Now());
      } else {
        w.b = Batch();
      }
    } catch (const std::exception& ex) {
      s_->fatal->Set(ex.what());   // the caller keeps draining the table so that the readers can finish
    }
  }
  if (!submitted_batch) s_->out->Deliver(g, OutBatch());
}

// Step 1: utterances of another width are warned about and counted; the others are listed where the reader left them (w->b
// keeps them alive until Finalize): the chunks are copied from there straight into the engine's pinned staging buffer
// (ExtractJob::StartPtrs) - one host copy per byte.
void Consumer::RejectWrongDimension(Work* w) {
  w->offs.assign(1, 0);
  w->idx.clear();
  w->uptr.clear();
  w->urows.clear();
  for (size_t i = 0; i < w->b.utts.size(); ++i) {
    const Utt& u = w->b.utts[i];
    if (u.feats.rows > 0 && u.feats.cols != D_) {
      std::ostringstream m;
      m << "feature dimension " << u.feats.cols << " of utterance " << u.key << " does not match the model's " << D_;
      (*s_->warn)(m.str());
      ++num_fail;
      continue;
    }
    w->uptr.push_back(u.feats.Data());
    w->urows.push_back(u.feats.rows);
    w->idx.push_back((int)i);
  }
}

// Step 2, front-end jobs: sliding CMN over the WHOLE utterance first, then the voiced frames (order of the two pipe stages).
// The device path takes raw rows - compressed views as they are - and nothing comes back but embeddings; a batch it cannot take
// with compressed views is tried again expanded; one that does not fit one forward batch takes the host round trip.
bool Consumer::SubmitFrontEnd(Work* w) {
  std::vector<int> keep_idx;
  std::vector<const float*> rawp, vadp;
  std::vector<int32_t> rrows;
  std::vector<const uint8_t*> cmp;    // compressed views of a mapped archive: expanded on the device (or below, on the host)
  std::vector<size_t> cmb;
  bool any_cm = false;
  for (int i : w->idx) {
    const Utt& u = w->b.utts[i];
    const int T = u.feats.rows;
    const std::vector<float>* v = nullptr;
    if (s_->vad) {
      VadVerdict verdict;
      {
        std::lock_guard<std::mutex> vlk(s_->vad_mu);
        verdict = JudgeVad(s_->vad, u.key, T);
      }
      if (!verdict.ok()) {
        (*s_->warn)(verdict.Warning(u.key, T));
        ++num_fail;
        continue;
      }
      v = verdict.decisions;
    }
    keep_idx.push_back(i);
    rawp.push_back(u.feats.cm ? nullptr : u.feats.Data());
    cmp.push_back(u.feats.cm);
    cmb.push_back(u.feats.cm_bytes);
    any_cm = any_cm || u.feats.cm != nullptr;
    vadp.push_back(v ? v->data() : nullptr);
    rrows.push_back(T);
  }
  w->idx.swap(keep_idx);
  const int n = (int)w->idx.size();
  if (!n) return false;
  bool submitted = w->job.StartFrontEnd(eng_, s_->opt, cur_, seq_, n, rawp.data(), rrows.data(), vadp.data(), any_cm ? cmp.data() : nullptr,
                                        any_cm ? cmb.data() : nullptr);
  if (submitted && any_cm) num_cm_device += n;
  if (!submitted && any_cm) {
    // the batch cannot go to the device as it is (an utterance cut into several chunks, a mixed batch): the compressed
    // views are expanded here, into the utterances themselves, and the float paths below see what they always saw
    for (int k = 0; k < n; ++k) {
      Utt& u = w->b.utts[w->idx[k]];
      if (!u.feats.cm) continue;
      Matrix full;
      ExpandCompressedView(u.feats, &full);
      u.feats = std::move(full);
      rawp[k] = u.feats.Data();
    }
    submitted = w->job.StartFrontEnd(eng_, s_->opt, cur_, seq_, n, rawp.data(), rrows.data(), vadp.data());
  }
  if (submitted) ++seq_;
  else FrontEndOnHost(w, rawp, vadp, rrows);
  return submitted;
}

// A batch that does not fit one forward batch: front-end result back to the host, then Start()
void Consumer::FrontEndOnHost(Work* w, const std::vector<const float*>& rawp, const std::vector<const float*>& vadp,
                              const std::vector<int32_t>& rrows) {
  ++num_fe_host;
  const int n = (int)w->idx.size();
  sel_row_.clear();
  sel_utt_.clear();
  poffs_.assign(1, 0);
  std::vector<int32_t> raw_off2(1, 0);
  std::vector<float> raw2;
  for (int k = 0; k < n; ++k) {
    const int T = rrows[k];
    const int32_t base = raw_off2.back();
    for (int t = 0; t < T; ++t)
      if (!vadp[k] || vadp[k][t] != 0.f) {
        sel_row_.push_back(base + t);
        sel_utt_.push_back(k);
      }
    raw2.insert(raw2.end(), rawp[k], rawp[k] + (size_t)T * D_);
    raw_off2.push_back(base + T);
    poffs_.push_back((int32_t)sel_row_.size());
  }
  processed_.resize(sel_row_.size() * (size_t)D_);
  eng_->FrontEndHost(raw2.data(), raw_off2.data(), n, sel_row_.data(), sel_utt_.data(), (int)sel_row_.size(), s_->opt.cmn_window,
                     s_->opt.cmn_center, s_->opt.cmn_min_window, processed_.data());
  w->packed.swap(processed_);
  w->offs = poffs_;
}

// Waits for the batch, applies the back-end and delivers its number (see Process).
void Consumer::Finalize(Work* w) {
  const ExtractOptions& opt = s_->opt;
  const int n = (int)w->idx.size();
  emb_.resize((size_t)n * E_);
  ok_.assign(n, 0);
  why_.assign(n, std::string());
  w->job.Finish(emb_.data(), ok_.data(), &why_);
  const float* vec = emb_.data();
  int VE = E_;
  if (n && has_backend_) {
    BackendOptions bo;
    bo.mean = opt.backend_mean.empty() ? nullptr : opt.backend_mean.data();
    bo.transform = opt.backend_transform.empty() ? nullptr : opt.backend_transform.data();
    bo.t_rows = opt.backend_t_rows;
    bo.t_cols = opt.backend_t_cols;
    bo.normalize = opt.backend_normalize;
    bo.scaleup = opt.backend_scaleup;
    VE = bo.transform ? bo.t_rows : E_;
    post_.resize((size_t)n * VE);
    for (int k = 0; k < n; ++k)
      if (!ok_[k]) std::fill(emb_.begin() + (size_t)k * E_, emb_.begin() + (size_t)(k + 1) * E_, 0.f);
    BackendApply(eng_->device(), emb_.data(), n, E_, bo, post_.data(), nullptr);
    vec = post_.data();
  }
  OutBatch ob;
  ob.VE = VE;
  ob.keys.reserve(n);
  ob.vecs.assign(vec, vec + (size_t)n * VE);
  ob.okv.resize(n);
  ob.whys.resize(n);
  ob.rows.resize(n);
  for (int k = 0; k < n; ++k) {
    Utt& u = w->b.utts[w->idx[k]];
    ob.keys.push_back(std::move(u.key));   // (the batch is dropped below)
    ob.okv[k] = ok_[k] ? 1 : 0;
    if (!ok_[k]) ob.whys[k] = why_[k];
    ob.rows[k] = u.feats.rows;
  }
  s_->source->Recycle(std::move(w->b));
  w->b = Batch();
  s_->out->Deliver(w->g, std::move(ob));
}

void Consumer::Drain() {
  for (int k = 1; k <= NS; ++k) {
    Work& w = work_[(cur_ + k) % NS];
    if (!w.job.active()) continue;
    if (s_->fatal->is_set()) {   // still owed to the ordered writer
      s_->out->Deliver(w.g, OutBatch());
      continue;
    }
    try {
      Finalize(&w);
    } catch (const std::exception& ex) {
      s_->fatal->Set(ex.what());
      s_->out->Deliver(w.g, OutBatch());
    }
  }
}

}  // namespace xv
