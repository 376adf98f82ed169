// Feature ingestion of the table loop.  See batch_source.h.
#include "batch_source.h"

#include <algorithm>

namespace xv {

namespace {
std::unique_ptr<MatrixTableIndexer> OpenIndexer(const std::string& rspecifier, int n_readers) {
  std::unique_ptr<MatrixTableIndexer> ix;
  if (n_readers > 1) {
    ix.reset(new MatrixTableIndexer(rspecifier));
    if (!ix->usable()) ix.reset();
  }
  return ix;
}
}  // namespace

BatchSource::BatchSource(const std::string& rspecifier, const BatchSourceOptions& opt, const WarnFn& warn)
    : rspecifier_(rspecifier),
      opt_(opt),
      warn_(warn),
      is_scp_(ParseRspecifier(rspecifier).is_scp),
      indexer_(OpenIndexer(rspecifier, opt.n_readers)),
      // indexed: what is planned and not taken is bounded by the credits, so neither queue ever makes a thread wait for room
      // (+ 1: the terminal batch of the first ReaderFailed; see there for a second one)
      queue_(indexer_ ? 2 * opt.n_readers + 3 : 2),
      plans_(2 * opt.n_readers + 3),
      credits_(2 * opt.n_readers + 2),
      threads_([this] { Stop(); }) {}

BatchSource::~BatchSource() {}

void BatchSource::Stop() {
  stop_ = true;
  queue_.Cancel();
  plans_.Cancel();
  credits_.Cancel();
}

void BatchSource::Finish() {
  Stop();
  threads_.Join();
}

void BatchSource::Start(TableIndex* index) {
  if (!indexer_) {
    threads_.Start(nullptr, [this] { Guarded(&BatchSource::StreamReader, "unknown error in the reader thread"); });
    return;
  }
  if (index && index->valid) pre_index_ = std::move(*index);
  for (int i = 0; i < 2 * opt_.n_readers + 2; ++i) credits_.Push(0);
  threads_.Start("xv-index", [this] { Guarded(&BatchSource::IndexPass, "unknown error in the index pass"); });
  for (int i = 0; i < opt_.n_readers; ++i)
    threads_.Start("xv-read", [this] { Guarded(&BatchSource::IndexedReader, "unknown error in a reader thread"); });
}

bool BatchSource::Next(Batch* b) {
  if (ended_ || !queue_.Pop(b)) return false;
  if (b->last) ended_ = true;
  else if (indexer_) credits_.Push(0);   // one more batch may be planned
  return true;
}

void BatchSource::Recycle(Batch&& b) {
  if (indexer_) return;   // views and whole-batch reads: nothing to reuse
  std::lock_guard<std::mutex> lk(pool_mu_);
  for (Utt& u : b.utts)
    if (pool_.size() < 4096 && u.feats.data.capacity()) pool_.push_back(std::move(u.feats.data));
}

// A matrix read into a buffer that is already large enough is not zero-filled first - for a pipe, whose single reader thread is
// the job's ceiling, that pass over every byte was a fifth of the thread's time.
void BatchSource::TakeBuffer(Matrix* m) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  if (m->data.capacity() == 0 && !pool_.empty()) {
    m->data = std::move(pool_.back());
    pool_.pop_back();
  }
}

// Anything that leaves a thread's body (an allocation failing while a batch is assembled) must not leave the thread: an
// exception escaping a std::thread is std::terminate.  It becomes the job's error, and a terminal batch releases whoever waits.
void BatchSource::Guarded(void (BatchSource::*body)(), const char* unknown) {
  try {
    (this->*body)();
  } catch (const std::exception& ex) {
    ReaderFailed(ex.what());
  } catch (...) {
    ReaderFailed(unknown);
  }
}

// Several threads may fail.  The queue has room for one terminal batch; Next() stops at the first, so a later one may wait in
// Push, and so may an index pass that goes on planning (Close does not stop a Push) - until Stop(), which Finish() and the
// destructor call before they join, cancels the queues.
void BatchSource::ReaderFailed(const char* what) {
  error_.Set(what);
  Batch b;
  b.last = true;
  queue_.Push(std::move(b));
  plans_.Close();   // the readers finish what is planned and end
}

void BatchSource::StreamReader() {
  try {
    SequentialMatrixReader rd(rspecifier_);
    Batch cur;
    long rows = 0;
    std::string key, e;
    Matrix m;
    TakeBuffer(&m);
    while (!stop_ && rd.Next(&key, &m, &e)) {
      if (!e.empty()) {
        warn_("failed to read features for " + key + ": " + e);
        ++num_fail_read_;
        continue;
      }
      if (ClosesBatch(opt_, cur.utts.size(), rows, m.rows)) {
        if (!queue_.Push(std::move(cur))) break;
        cur = Batch();
        rows = 0;
      }
      Utt u;
      u.key = key;
      u.feats = std::move(m);
      rows += u.feats.rows;
      cur.utts.push_back(std::move(u));
      m = Matrix();
      TakeBuffer(&m);
    }
    reader_status_ = rd.Close();
    cur.last = true;
    queue_.Push(std::move(cur));
  } catch (const std::exception& ex) {   // a damaged archive: what was delivered stays delivered, the open batch is dropped
    error_.Set(ex.what());
    Batch b;
    b.last = true;
    queue_.Push(std::move(b));
  }
}

// The calibration's index of the table, when there is one (it is consumed: entries are moved out), else the indexer.
bool BatchSource::NextEntry(MatrixTableIndexer::Entry* e) {
  if (!pre_index_.valid) return indexer_->Next(e);
  if (pre_i_ < pre_index_.entries.size()) {
    *e = std::move(pre_index_.entries[pre_i_++]);
    return true;
  }
  if (!pre_index_.error.empty()) throw KioError(pre_index_.error);   // where that index stopped: reported after what precedes it
  return false;
}

// Batches by the rule of the stream reader, from the headers (objects whose size is not known without reading them - text,
// pipes - count as 0 rows: such batches are bounded by max_utts only, and the extractor splits what does not fit one forward
// pass).  What stops the index early ends the table there: the open batch is still read and delivered.
void BatchSource::IndexPass() {
  Plan cur;
  long rows = 0, next_seq = 0;
  auto push = [&](bool last) {
    char credit;
    if (!credits_.Pop(&credit)) return;   // stopped
    cur.last = last;
    cur.seq = next_seq++;
    plans_.Push(std::move(cur));
    cur = Plan();
    rows = 0;
  };
  try {
    MatrixTableIndexer::Entry e;
    while (!stop_ && NextEntry(&e)) {
      if (!e.error.empty()) {
        warn_("failed to read features for " + e.key + ": " + e.error);
        ++num_fail_read_;
        continue;
      }
      const int r = std::max(e.rows, 0);
      if (ClosesBatch(opt_, cur.entries.size(), rows, r)) push(false);
      rows += r;
      cur.entries.push_back(std::move(e));
    }
  } catch (const std::exception& ex) {
    error_.Set(ex.what());
  }
  push(true);
  plans_.Close();
}

void BatchSource::IndexedReader() {
  ArchiveCursor cursor;
  Plan pb;
  while (plans_.Pop(&pb)) {
    Batch b;
    b.last = pb.last;
    for (MatrixTableIndexer::Entry& e : pb.entries) {
      Utt u;
      try {
        // a float matrix in a regular file is not read at all: the utterance is a view of the mapped archive, and its bytes
        // are touched once, by the copy into the pinned staging buffer
        if (!opt_.views || !mapper_.View(e, &u.feats, opt_.compressed_views)) ReadIndexedMatrix(e, &cursor, &u.feats);
      } catch (const std::exception& ex) {
        if (e.offset >= 0 && !is_scp_) {   // a damaged archive is fatal, as in the stream reader
          error_.Set(ex.what());
          continue;
        }
        warn_("failed to read features for " + e.key + ": " + ex.what());
        ++num_fail_read_;
        continue;
      }
      u.key = std::move(e.key);
      b.utts.push_back(std::move(u));
    }
    // sequencer: whatever is next in table order goes to Next()'s queue
    filled_.Put(pb.seq, std::move(b), [this](Batch&& next) { queue_.Push(std::move(next)); });
  }
}

}  // namespace xv
