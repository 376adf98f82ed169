// Table-driven extraction loop.  See table_extract.h.  The pieces: batch_source.h (feature ingestion), table_calibrate.h (the
// arithmetic of the job), table_consumer.h (one consumer per engine, the ordered writer), stage_pipeline.h (the threading).
#include "table_extract.h"

#include <dirent.h>
#include <sys/resource.h>
#include <sys/time.h>

#include <chrono>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>

#include "knobs.h"
#include "table_calibrate.h"
#include "table_consumer.h"

namespace xv {

namespace {

typedef std::chrono::steady_clock::time_point TimePoint;
double SecsSince(TimePoint t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// XVEC_TIMING: where the consumers' time went, and what the front-end did with the batches
void ReportStages(const std::vector<std::unique_ptr<Consumer>>& cons, double t_wait, const LogFn& log) {
  double t_pack = 0, t_start = 0, t_fin = 0;
  long n_cm = 0, n_feh = 0;
  for (const auto& C : cons) {
    t_pack += C->t_pack;
    t_start += C->t_start;
    t_fin += C->t_fin;
    n_cm += C->num_cm_device;
    n_feh += C->num_fe_host;
  }
  std::ostringstream m;
  m << "consumer stages" << (cons.size() > 1 ? " (summed over the engines' threads)" : "") << ": wait for reader " << t_wait << " s, pack "
    << t_pack << " s, plan+submit " << t_start << " s, finish+write " << t_fin << " s";
  log("LOG", m.str());
  if (n_cm) log("LOG", "front-end: " + std::to_string(n_cm) + " utterances went to the device compressed (one byte per element) and were expanded there");
  if (n_feh) log("LOG", "front-end: " + std::to_string(n_feh) + " batches did not fit one forward batch and took the host round trip");
}

// XVEC_TIMING: host budget of the table loop - CPU seconds of ALL threads of the process (readers, copy threads, consumers,
// writer, the runtime's own) between the first batch and the last write, what eight ranks on one node have to share - and who
// spent it: CPU seconds per thread NAME since the threads were created (/proc/self/task/*/schedstat; the HIP runtime's own
// threads carry the process name).
void ReportHostCost(const struct rusage& ru0, TimePoint t0, long n_all, const LogFn& log) {
  struct rusage ru1;
  getrusage(RUSAGE_SELF, &ru1);
  auto tv = [](const timeval& a, const timeval& b) { return (double)(b.tv_sec - a.tv_sec) + 1e-6 * (double)(b.tv_usec - a.tv_usec); };
  const double user = tv(ru0.ru_utime, ru1.ru_utime), sys = tv(ru0.ru_stime, ru1.ru_stime);
  const double wall = SecsSince(t0);
  std::ostringstream h;
  h.precision(4);
  h << "host cost of the table loop: " << user << " s user + " << sys << " s system over " << wall << " s = " << (user + sys) / std::max(wall, 1e-9)
    << " cores; " << (n_all ? 1e6 * (user + sys) / n_all : 0.0) << " us of CPU per utterance (" << n_all << " utterances, "
    << (ru1.ru_minflt - ru0.ru_minflt) << " minor page faults)";
  log("LOG", h.str());
  std::map<std::string, std::pair<double, int>> by_name;
  if (DIR* d = opendir("/proc/self/task")) {
    while (dirent* de = readdir(d)) {
      if (de->d_name[0] == '.') continue;
      const std::string base = std::string("/proc/self/task/") + de->d_name;
      std::ifstream c(base + "/comm"), st(base + "/schedstat");
      std::string name;
      unsigned long long ns = 0;
      if (std::getline(c, name) && (st >> ns)) {
        by_name[name].first += 1e-9 * (double)ns;
        by_name[name].second += 1;
      }
    }
    closedir(d);
  }
  std::ostringstream t;
  t.precision(3);
  t << "CPU seconds by thread name (threads):";
  for (const auto& kv : by_name) t << " " << kv.first << " " << kv.second.first << " (" << kv.second.second << ")";
  log("LOG", t.str());
}

}  // namespace

TableExtractResult RunTableExtraction(Engine* engine, const ExtractOptions& opt, const std::string& feat_rspec,
                                      const std::string& vec_wspec, const LogFn& log) {
  return RunTableExtraction(std::vector<Engine*>(1, engine), opt, feat_rspec, vec_wspec, log);
}

// Several engines = several GPUs driven by this one process (nnet3-xvector-compute --devices=..., the `--nj 1` form of
// extract_xvectors_new.sh:83-93).  Whole batches are dealt to the engines round-robin in table order - one consumer thread
// each: the packing of a batch (one host copy per byte) and the wait for its device are what a single thread could not do for
// more than one GPU - and the calling thread writes what they finalise in that order: the output archive is byte-identical
// to a one-GPU run of the same job.  With ONE engine its consumer runs on the calling thread and writes what it finalises
// there: no thread is started, no batch waits in the reorder buffer.  The arithmetic is chosen once, on engines[0], and applied
// to the others (like rank 0's choice in dist_extract.py).
TableExtractResult RunTableExtraction(const std::vector<Engine*>& engines, const ExtractOptions& opt, const std::string& feat_rspec,
                                      const std::string& vec_wspec, const LogFn& log) {
  if (engines.empty() || !engines[0]) throw EngineError("RunTableExtraction: no engine");
  Engine* const engine = engines[0];   // calibration, back-end dimensions
  const int NE = (int)engines.size();
  for (Engine* e : engines)
    if (!e || e->info().input_dim != engine->info().input_dim || e->info().output_dim != engine->info().output_dim ||
        e->can_switch_fast_mode() != engine->can_switch_fast_mode())
      throw EngineError("RunTableExtraction: the engines do not hold the same model");
  TableExtractResult res;
  const int E = engine->info().output_dim;
  // Everything that can fail on a user error - an option that does not fit the model, an unreadable VAD table, an unwritable
  // output, a feature table that is not there - fails here, before a thread or a measurement exists.  What can still throw
  // afterwards unwinds through the thread groups of the source and of the consumers, which release and join their threads.
  if (!opt.backend_mean.empty() && (int)opt.backend_mean.size() != E)
    throw KioError("--backend-mean has dimension " + std::to_string(opt.backend_mean.size()) + ", the embedding has " +
                   std::to_string(E));
  if (!opt.backend_transform.empty() && opt.backend_t_cols != E && opt.backend_t_cols != E + 1)
    throw KioError("Dimension mismatch: the embedding has dimension " + std::to_string(E) + " and --backend-transform has " +
                   std::to_string(opt.backend_t_cols) + " columns");
  const bool use_frontend = opt.cmn_window > 0 || !opt.vad_rspecifier.empty();
  std::unique_ptr<RandomAccessVectorReader> vad;
  if (!opt.vad_rspecifier.empty()) vad.reset(new RandomAccessVectorReader(opt.vad_rspecifier));
  TableWriter writer(vec_wspec);
  Warner warn(log);
  BatchSourceOptions so;
  so.max_rows = opt.max_batch_rows;
  so.max_utts = opt.max_batch_chunks;
  so.n_readers = std::max(1, std::min(16, DebugKnobInt("readers", std::min(16, 4 * NE))));
  so.views = DebugKnobInt("mmap", 1) != 0;
  so.compressed_views = use_frontend && DebugKnobInt("cm_on_device", 1) != 0;   // compressed matrices of a front-end job: expanded on the GPU
  BatchSource source(feat_rspec, so, std::ref(warn));   // (holds the mapped files: declared before whoever holds a batch)

  ArithmeticChoice choice(engines, opt, log, std::ref(warn));
  choice.ReadFromFile();
  TableIndex index;
  if (choice.pending() && source.addressable()) choice.MeasureOnTable(feat_rspec, &index);
  source.Start(&index);

  const TimePoint t0 = std::chrono::steady_clock::now();
  struct rusage ru0;
  getrusage(RUSAGE_SELF, &ru0);
  OrderedWriter out(&writer, &warn, &res, /*direct=*/NE == 1);
  FirstError fatal([&out] { out.Interrupt(); });
  ConsumerShared shared{opt, vad.get(), &source, &out, &fatal, &warn, {}};
  std::vector<std::unique_ptr<Consumer>> cons;
  for (Engine* e : engines) cons.emplace_back(new Consumer(e, &shared));
  typedef BoundedQueue<std::pair<long, Batch>> Inbox;   // several engines: two batches wait in front of each consumer
  std::vector<std::unique_ptr<Inbox>> inbox;
  ThreadGroup workers([&inbox] {   // closed, not cancelled: what was dealt out is still processed and delivered
    for (auto& q : inbox) q->Close();
  });
  for (int e = 0; NE > 1 && e < NE; ++e) {
    inbox.emplace_back(new Inbox(2));
    workers.Start(nullptr, [c = cons[e].get(), q = inbox[e].get()] { c->Run(q); });
  }
  long next_g = 0;   // batches are numbered in table order as they are dealt out
  auto dispatch = [&](Batch&& b) {
    const long g = next_g++;
    if (NE == 1) return cons[0]->Process(std::move(b), g);   // (writes what it finalises itself)
    inbox[g % NE]->Push(std::make_pair(g, std::move(b)));
    out.WriteReady();
  };
  double t_wait = 0;   // XVEC_TIMING: waiting for the readers
  for (;;) {
    Batch b;
    const TimePoint tw0 = std::chrono::steady_clock::now();
    if (!source.Next(&b)) break;
    t_wait += SecsSince(tw0);
    if (!choice.pending()) {
      dispatch(std::move(b));
      continue;
    }
    // a stream is calibrated on its head: nothing is submitted before the arithmetic of the whole job is chosen
    for (Batch& hb : choice.MeasureOnStreamHead(std::move(b), &fatal)) dispatch(std::move(hb));
  }
  if (NE == 1) {
    cons[0]->Drain();
  } else {
    for (auto& q : inbox) q->Close();
    out.WriteUntil(next_g);   // write while the consumers finish
    workers.Join();
  }
  out.WriteRest();   // (gaps only after a fatal error)
  for (const auto& C : cons) res.num_fail += C->num_fail;
  if (getenv("XVEC_TIMING")) {
    ReportStages(cons, t_wait, log);
    ReportHostCost(ru0, t0, res.num_success + res.num_fail, log);
  }
  source.Finish();
  writer.Close();
  if (fatal.is_set()) throw std::runtime_error(fatal.what());
  if (!source.error().empty()) throw KioError(source.error());
  res.num_fail += source.num_fail_read();
  res.reader_status = source.reader_status();
  res.seconds = SecsSince(t0);
  return res;
}

}  // namespace xv
