// The device side of the table loop (table_extract.cc): one Consumer per engine takes batches, runs them and hands what it
// finalises to the one OrderedWriter, which writes in table order on the calling thread.
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "batch_source.h"
#include "stage_pipeline.h"
#include "table_extract.h"

namespace xv {

// Readers, consumers and the writer warn from their own threads: one line at a time.
class Warner {
 public:
  explicit Warner(const LogFn& log) : log_(log) {}
  void operator()(const std::string& m) {
    std::lock_guard<std::mutex> lk(mu_);
    log_("WARNING", m);
  }

 private:
  const LogFn& log_;
  std::mutex mu_;
};

// What a finalised batch hands to the writer: one record per utterance that reached the device, in table order.
struct OutBatch {
  std::vector<std::string> keys;
  std::vector<float> vecs;   // [keys.size()][VE]
  int VE = 0;
  std::vector<char> okv;
  std::vector<std::string> whys;
  std::vector<int> rows;
};

// Batches are numbered in table order.  EVERY number is delivered exactly once, by whoever holds the batch (an empty record
// when nothing of it reaches the archive), so the writer never waits for a number that does not come; should a failure keep
// one back all the same, Interrupt() releases the wait and WriteRest() writes what is there.
// direct (the one-engine job: its consumer runs on the writing thread and finalises in table order): Deliver writes at once.
// The write is then part of the consumer's "finish+write" time, and what it throws is caught where the consumer's own failures
// are and becomes the job's fatal error; with several engines it leaves the calling thread at once.
class OrderedWriter {
 public:
  OrderedWriter(TableWriter* writer, Warner* warn, TableExtractResult* res, bool direct)
      : writer_(writer), warn_(warn), res_(res), direct_(direct) {}
  void Deliver(long g, OutBatch&& ob) {   // any thread (direct: the writing thread)
    if (direct_) Write(ob);
    else done_.Put(g, std::move(ob));
  }
  void Interrupt() { done_.Interrupt(); }                                // any thread
  // the calling thread of the job:
  void WriteReady() {   // whatever is next in table order
    OutBatch ob;
    while (done_.TakeNext(&ob)) Write(ob);
  }
  void WriteUntil(long n) {   // ... waiting, until n batches are written or the wait is interrupted
    OutBatch ob;
    while (done_.next() < n && done_.WaitNext(&ob)) Write(ob);
  }
  void WriteRest() {   // whatever is there, gaps included
    OutBatch ob;
    while (done_.TakeAny(&ob)) Write(ob);
  }

 private:
  void Write(const OutBatch& ob) {
    for (size_t k = 0; k < ob.keys.size(); ++k) {
      if (!ob.okv[k]) {
        (*warn_)(ob.whys[k] + ": " + ob.keys[k]);
        ++res_->num_fail;
        continue;
      }
      writer_->WriteVec(ob.keys[k], ob.vecs.data() + k * (size_t)ob.VE, ob.VE);
      res_->frames += ob.rows[k];
      ++res_->num_success;
    }
  }
  TableWriter* const writer_;
  Warner* const warn_;
  TableExtractResult* const res_;
  const bool direct_;
  ReorderBuffer<OutBatch> done_;
};

// What the consumers of a job share.  The VAD reader caches what it loads: one consumer at a time, behind vad_mu.
struct ConsumerShared {
  const ExtractOptions& opt;
  RandomAccessVectorReader* vad;   // null: none
  BatchSource* source;             // finished batches go back to it
  OrderedWriter* out;
  FirstError* fatal;
  Warner* warn;
  std::mutex vad_mu;
};

// One engine (= one GPU) of a table job: its ring of host slots, scratch, counters and timers.  Up to kNumHostSlots batches are
// queued on the device (ExtractJob::Start returns at once): after submitting batch i the consumer finalises batch i-2 (average,
// back-end, hand over to the writer) and packs batch i+1 while i-1 and i keep the GPU busy - with only two, both lanes ran
// their batches side by side, finished together, and the GPU idled while the host caught up (measured: 20 % idle).
class Consumer {
 public:
  Consumer(Engine* engine, ConsumerShared* shared);
  // One batch: reject what cannot run, select the front-end path, submit; then finalise the oldest batch in flight.  Never
  // throws what the extraction throws: that becomes the job's fatal error, and batch g is delivered empty.
  void Process(Batch&& b, long g);
  void Drain();   // the batches still in flight, oldest first
  // the thread of a several-engine job: Process until the inbox is closed, then Drain
  void Run(BoundedQueue<std::pair<long, Batch>>* inbox);

  long num_fail = 0;        // utterances rejected before they reached the device
  long num_cm_device = 0;   // utterances that went up compressed and were expanded on the device
  long num_fe_host = 0;     // batches of a front-end job that had to take the host round trip
  double t_pack = 0, t_start = 0, t_fin = 0;

 private:
  struct Work {
    Batch b;
    long g = 0;                  // number of the batch in table order
    std::vector<int> idx;        // utterances of b that entered the device batch
    std::vector<float> packed;   // front-end path only: the processed rows, back to back
    std::vector<int32_t> offs;
    std::vector<const float*> uptr;   // plain path: rows of the utterances where the reader left them
    std::vector<int32_t> urows;
    ExtractJob job;
  };
  void RejectWrongDimension(Work* w);
  bool SubmitFrontEnd(Work* w);   // true: the batch is on the device; false: w->packed / offs hold the front-end's result, or w->idx is empty
  void FrontEndOnHost(Work* w, const std::vector<const float*>& rawp, const std::vector<const float*>& vadp, const std::vector<int32_t>& rrows);
  void Finalize(Work* w);

  Engine* const eng_;
  ConsumerShared* const s_;
  const int D_, E_;
  const bool use_frontend_, has_backend_;
  std::vector<Work> work_;
  int cur_ = 0;
  long seq_ = 0;   // running batch number on this engine (selects its lane)
  std::vector<int32_t> sel_row_, sel_utt_, poffs_;
  std::vector<float> processed_, emb_, post_;
  std::vector<int32_t> ok_;
  std::vector<std::string> why_;
};

}  // namespace xv
