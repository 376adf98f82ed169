// The arithmetic of a table job, chosen once before anything is submitted (table_extract.cc): read from the recipe's shared
// file, or measured - on a sample spread over an addressable table, or on the head of a stream - on engines[0], applied to the
// other engines, and with a shared file published and read back (calib_file.h: this job's choice or that of the job that
// published first).
#pragma once
#include <deque>
#include <string>
#include <vector>

#include "batch_source.h"
#include "calib_file.h"
#include "stage_pipeline.h"
#include "table_extract.h"

namespace xv {

class ArithmeticChoice {
 public:
  ArithmeticChoice(const std::vector<Engine*>& engines, const ExtractOptions& opt, const LogFn& log, const BatchSource::WarnFn& warn);   // warn: locks for itself
  // A shared file that exists is applied, and nothing is left to measure.  Says so in the log when the choice will be this
  // job's alone.
  void ReadFromFile();
  bool pending() const { return pending_; }   // a measurement is still to be made: no batch may be submitted
  // Addressable table: the sample is spread over the whole list, drawn before the readers start; *index receives the index for
  // them.  An unreadable sample (KioError) is not the job's failure: the packed arithmetic stays and the extraction reports
  // the bad object itself, after writing the good ones.  Anything else - a device fault in a candidate arithmetic, a
  // stream-K time-out, a failed allocation - is thrown: swallowed, it let independent jobs over one table run different
  // arithmetics and exit 0.
  void MeasureOnTable(const std::string& feat_rspec, TableIndex* index);
  // Stream: batches are held back until calibrate_utts utterances have arrived (whatever the batch size, so that the choice -
  // and with it every embedding - does not depend on --batch-frames) or the stream has ended; then the measurement is made on
  // them (a failure becomes *fatal) and they are returned, in order, to be dispatched.  Empty: still holding.
  std::deque<Batch> MeasureOnStreamHead(Batch&& b, FirstError* fatal);

 private:
  void ShareChoice();   // what engines[0] was set to, on every other engine
  void Adopt(const SharedChoice& sc, const std::string& how);
  void Publish(const Engine::Calibration* c, const std::string& sample);   // after a measurement (or a failed one: c = null)

  const std::vector<Engine*>& engines_;
  Engine* const engine_;
  const ExtractOptions& opt_;
  const LogFn& log_;
  const BatchSource::WarnFn warn_;
  const bool shared_;
  bool pending_ = false;
  std::deque<Batch> held_;
  size_t held_utts_ = 0;
};

}  // namespace xv
