#include "feat_batch.h"

#include <string.h>

#include "cli.h"

namespace xv {

struct FeatBatchReader::Impl {
  int64_t max_frames;
  bool allow_cm;
  std::unique_ptr<MatrixTableIndexer> indexer;
  std::unique_ptr<SequentialMatrixReader> seq;
  FileMapper mapper;
  ArchiveCursor cursor;
  // the matrix that did not fit the batch before
  bool held = false;
  std::string held_key;
  Matrix held_m;
  bool done = false;

  // the next readable matrix with rows; false at the end
  bool Read(std::string* key, Matrix* m, std::vector<Problem>* problems) {
    for (;;) {
      std::string err;
      if (indexer) {
        MatrixTableIndexer::Entry e;
        if (!indexer->Next(&e)) return false;
        *key = e.key;
        if (!e.error.empty()) {
          err = e.error;
        } else {
          try {
            *m = Matrix();
            if (!mapper.View(e, m, allow_cm)) ReadIndexedMatrix(e, &cursor, m);
          } catch (const std::exception& ex) {
            err = ex.what();
          }
        }
      } else {
        *m = Matrix();
        if (!seq->Next(key, m, &err)) return false;
      }
      if (!err.empty()) {
        problems->push_back(Problem{*key, err});
        continue;
      }
      if (m->rows == 0 || m->cols == 0) {
        problems->push_back(Problem{*key, ""});
        continue;
      }
      if (m->cm && m->cols > 64) {   // wider than the device expansion takes: the floats are made here
        Matrix full;
        ExpandCompressedView(*m, &full);
        *m = std::move(full);
      }
      return true;
    }
  }
};

FeatBatchReader::FeatBatchReader(const std::string& rspecifier, int64_t max_frames, bool allow_compressed) : impl_(new Impl) {
  impl_->max_frames = max_frames;
  impl_->allow_cm = allow_compressed;
  impl_->indexer.reset(new MatrixTableIndexer(rspecifier));
  if (!impl_->indexer->usable()) {
    impl_->indexer.reset();
    impl_->seq.reset(new SequentialMatrixReader(rspecifier));
  }
}

FeatBatchReader::~FeatBatchReader() {}

bool FeatBatchReader::Next(Batch* b, std::vector<Problem>* problems) {
  Impl& I = *impl_;
  *b = Batch();
  b->row_off.assign(1, 0);
  if (I.done) return false;
  for (;;) {
    std::string key;
    Matrix m;
    if (I.held) {
      key = std::move(I.held_key);
      m = std::move(I.held_m);
      I.held = false;
    } else if (!I.Read(&key, &m, problems)) {
      I.done = true;
      break;
    }
    const bool cm = m.cm != nullptr;
    if (!b->keys.empty() && (m.cols != b->cols || cm != b->compressed)) {   // a batch has one width and one kind
      I.held = true;
      I.held_key = std::move(key);
      I.held_m = std::move(m);
      break;
    }
    b->cols = m.cols;
    b->compressed = cm;
    b->keys.push_back(std::move(key));
    if (cm) {
      b->cm_off.push_back((int64_t)b->cm.size());
      b->cm.insert(b->cm.end(), m.cm, m.cm + m.cm_bytes);
    } else {
      const size_t at = b->feats.size(), count = (size_t)m.rows * m.cols;
      b->feats.resize(at + count);
      memcpy(b->feats.data() + at, m.Data(), count * 4);   // (a view of a mapped archive has the archive's alignment)
    }
    b->max_rows = m.rows > b->max_rows ? m.rows : b->max_rows;
    b->row_off.push_back(b->row_off.back() + m.rows);
    if (b->row_off.back() >= I.max_frames) break;
  }
  return !b->keys.empty();
}

long FeatBatchWalk::Run(const std::function<void(const FeatBatchReader::Batch&)>& each) {
  FeatBatchReader::Batch b;
  std::vector<FeatBatchReader::Problem> problems;
  long num_err = 0;
  for (bool more = true; more;) {
    problems.clear();
    more = reader_.Next(&b, &problems);
    for (const auto& p : problems) {
      if (p.what.empty()) {
        if (policy_ == FeatProblems::kThrowUnreadable) continue;
        XWARN("Empty feature matrix for utterance " << p.key);
        if (policy_ == FeatProblems::kCount) ++num_err;
      } else {
        const std::string msg = "Failed to read features for key " + p.key + ": " + p.what;
        if (policy_ == FeatProblems::kThrowUnreadable) throw KioError(msg);
        XWARN(msg);
        ++num_err;
      }
    }
    if (more) each(b);
  }
  return num_err;
}

}  // namespace xv
