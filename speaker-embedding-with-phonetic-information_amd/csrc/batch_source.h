// Feature ingestion of the table loop (table_extract.cc): a feature table in, batches of utterances out, in table order.
//
// Tables whose objects can be addressed (binary archive in a regular file, script file of path:offset entries) are read by
// several threads: one index pass ("xv-index") forms the batches from the headers alone (MatrixTableIndexer: no data touched),
// the readers ("xv-read") fill whole batches, a sequencer hands them on in table order.  One thread parsing 7 GB/s of archive
// was what the loop waited for 42 % of the time.  Streams (pipes, standard input - the feature pipeline of
// extract_xvectors_new.sh:79) can only be read front to back: one reader thread.  The caller sees neither: Next() until false.
//
// What is held in memory: on the indexed path at most 2 * n_readers + 2 batches are planned and not yet taken by Next(); on
// the stream path 2 batches wait in the queue.  A damaged archive is fatal (error()); a bad entry of a script file is a
// warning and a count (num_fail_read()).  Whatever a reader thread throws becomes error(), after the batches in front of it
// have been delivered.  Nothing here names the device, the engine or the extractor's options.
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kio.h"
#include "stage_pipeline.h"

namespace xv {

struct Utt {
  std::string key;
  Matrix feats;
};
struct Batch {
  std::vector<Utt> utts;
  bool last = false;   // the table ends with this batch (which may be empty)
};

// The index of an addressable table - every entry, those with an error included, and the message of whatever stopped the
// indexing early - as the calibration's sample leaves it (table_extract.h CalibrateOnTable) for the batching pass to reuse.
struct TableIndex {
  bool valid = false;
  std::vector<MatrixTableIndexer::Entry> entries;
  std::string error;
};

struct BatchSourceOptions {
  int max_rows = 1 << 17;   // a batch never exceeds it unless a single utterance does
  int max_utts = 4096;
  int n_readers = 4;        // 1: the table is read front to back, whatever it is
  bool views = true;        // float matrices of a regular file are views of the mapped file, not copies
  bool compressed_views = false;   // ... and "CM" objects compressed views (kio.h Matrix::cm)
};

// THE batching rule, of both paths: whether an utterance of `rows` rows (0: not known without reading it) closes the batch that
// holds n_utts utterances and n_rows rows before it enters.
inline bool ClosesBatch(const BatchSourceOptions& o, size_t n_utts, long n_rows, int rows) {
  return n_utts > 0 && (n_rows + rows > o.max_rows || (int)n_utts >= o.max_utts);
}

class BatchSource {
 public:
  typedef std::function<void(const std::string&)> WarnFn;   // called from the reader threads: must lock for itself
  // Opens the table when it is to be indexed: a user error (no such file) is thrown here, before any thread exists.
  BatchSource(const std::string& rspecifier, const BatchSourceOptions& opt, const WarnFn& warn);
  ~BatchSource();   // stops and joins the threads; the mapped files go last
  bool addressable() const { return indexer_ != nullptr; }   // the indexed path will run
  // Starts the threads.  index (optional, valid): an index of this table that is consumed instead of indexing it again.
  void Start(TableIndex* index = nullptr);
  bool Next(Batch* b);        // false: the batch with `last` has been delivered before
  void Recycle(Batch&& b);    // a finished batch: the stream reader reuses its feature buffers (at most 4096 are kept)
  // valid once Next() has returned false, or after Finish()
  void Finish();              // stops and joins the threads
  long num_fail_read() const { return num_fail_read_; }
  int reader_status() const { return reader_status_; }      // exit status of an input pipe
  std::string error() const { return error_.what(); }       // empty: none

 private:
  struct Plan {
    long seq = 0;
    std::vector<MatrixTableIndexer::Entry> entries;
    bool last = false;
  };
  void Stop();
  void Guarded(void (BatchSource::*body)(), const char* unknown);
  void StreamReader();
  void IndexPass();
  bool NextEntry(MatrixTableIndexer::Entry* e);
  void IndexedReader();
  void ReaderFailed(const char* what);
  void TakeBuffer(Matrix* m);

  const std::string rspecifier_;
  const BatchSourceOptions opt_;
  const WarnFn warn_;
  const bool is_scp_;
  FileMapper mapper_;   // declared before everything that can hold a view of its mappings
  std::unique_ptr<MatrixTableIndexer> indexer_;
  TableIndex pre_index_;
  size_t pre_i_ = 0;
  BoundedQueue<Batch> queue_;     // to Next(), in table order
  BoundedQueue<Plan> plans_;      // index pass -> readers
  BoundedQueue<char> credits_;    // one per batch that may still be planned: taken by the index pass, given back by Next()
  ReorderBuffer<Batch> filled_;   // readers -> sequencer, by batch number
  std::mutex pool_mu_;
  std::vector<std::vector<float>> pool_;   // under pool_mu_
  std::atomic<bool> stop_{false};
  std::atomic<long> num_fail_read_{0};
  std::atomic<int> reader_status_{0};
  FirstError error_;
  bool ended_ = false;   // Next() only
  ThreadGroup threads_;  // last: joined before anything above goes
};

}  // namespace xv
