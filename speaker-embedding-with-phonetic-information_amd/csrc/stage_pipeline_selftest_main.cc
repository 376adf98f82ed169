// Stand-alone check of stage_pipeline.h, meant to be built with a sanitizer (make sanitize-pipeline: once with
// -fsanitize=thread, once with -fsanitize=address,undefined) and run on a machine without a GPU: a few hundred items through
// the three stages with stages of uneven speed, then the same with a stage that throws at a chosen item, for every stage and
// for the first, a middle and the last item.  Checks: every item arrives, in order, with what each stage did to it; a throw
// comes back out of RunThreeStages as that exception, after both threads were joined (the function returned), nothing at or
// behind the failing item was consumed, and everything in front of an item the reader failed on was.  Then the other primitives
// of the header in the shape of the x-vector table loop (TableLoop below).  Exit status 0 and "stage_pipeline selftest: ok" when
// all of it holds.
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "stage_pipeline.h"

namespace {

struct Item {
  int id = -1;
  std::vector<int> payload;   // heap memory that moves through the queues
  long worked = 0;
};

std::atomic<int> g_failures(0);
void Expect(bool ok, const std::string& what) {
  if (ok) return;
  fprintf(stderr, "FAILED: %s\n", what.c_str());
  ++g_failures;
}

// throw_stage: 0 none, 1 produce, 2 work, 3 consume; at item throw_at.  slow: which stage sleeps now and then.
void Run(int n, int throw_stage, int throw_at, int slow) {
  const std::string tag = "n=" + std::to_string(n) + " throw_stage=" + std::to_string(throw_stage) + " at=" + std::to_string(throw_at) +
                          " slow=" + std::to_string(slow);
  int next = 0;
  std::vector<int> seen;
  std::atomic<int> live(0);   // threads inside a stage function
  auto nap = [&](int stage, int id) {
    if (slow == stage && id % 7 == 0) std::this_thread::sleep_for(std::chrono::microseconds(200));
  };
  bool thrown = false;
  std::string what;
  try {
    xv::RunThreeStages<Item>(
        [&](Item* it) {
          ++live;
          const int id = next;
          if (throw_stage == 1 && id == throw_at) {
            --live;
            throw std::runtime_error("produce " + std::to_string(id));
          }
          if (id >= n) {
            --live;
            return false;
          }
          ++next;
          it->id = id;
          it->payload.assign(16 + id % 5, id);
          nap(1, id);
          --live;
          return true;
        },
        [&](Item* it) {
          ++live;
          if (throw_stage == 2 && it->id == throw_at) {
            --live;
            throw std::runtime_error("work " + std::to_string(it->id));
          }
          for (int v : it->payload) it->worked += v;
          nap(2, it->id);
          --live;
        },
        [&](Item* it) {
          ++live;
          if (throw_stage == 3 && it->id == throw_at) {
            --live;
            throw std::runtime_error("consume " + std::to_string(it->id));
          }
          Expect(it->worked == (long)it->id * (16 + it->id % 5), tag + ": item " + std::to_string(it->id) + " did not pass the work stage");
          seen.push_back(it->id);
          nap(3, it->id);
          --live;
        });
  } catch (const std::runtime_error& e) {
    thrown = true;
    what = e.what();
  }
  Expect(live.load() == 0, tag + ": a stage was still running when RunThreeStages returned");
  for (size_t i = 0; i < seen.size(); ++i) Expect(seen[i] == (int)i, tag + ": item " + std::to_string(seen[i]) + " arrived in place " + std::to_string(i));
  if (throw_stage == 0) {
    Expect(!thrown, tag + ": unexpected exception " + what);
    Expect((int)seen.size() == n, tag + ": " + std::to_string(seen.size()) + " items arrived");
  } else {
    const char* names[] = {"", "produce ", "work ", "consume "};
    Expect(thrown && what == names[throw_stage] + std::to_string(throw_at), tag + ": expected the stage's exception, got '" + what + "'");
    Expect((int)seen.size() <= throw_at, tag + ": items at or behind the failing one were consumed");
    if (throw_stage == 1) Expect((int)seen.size() == throw_at, tag + ": the items produced before the reader failed were not all consumed");
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The shape of the x-vector table loop (table_extract.cc, batch_source.cc) on the same primitives: an index thread plans
// numbered items under a credit bound, R readers complete them out of order, a sequencer (ReorderBuffer + sink) restores the
// order, the calling thread deals them round-robin to M consumers (M = 1: it is the consumer itself, and no thread is
// started for it), which deliver every number exactly once to the ordered writer on the calling thread.
// stage: 0 none, 1 a reader meets an unreadable item (recorded, the item arrives empty, reading goes on, reported at the end),
// 2 a consumer throws (fatal: everything after it is delivered empty), 3 the writer throws on the calling thread (unwinds
// through both thread groups).
struct LoopItem {
  long seq = 0;
  bool last = false, bad = false;
  std::vector<int> payload;
};
struct LoopOut {
  int id = -1;   // -1: an empty record
  long worked = 0;
};
struct Busy {   // a thread inside its body
  explicit Busy(std::atomic<int>* n) : n_(n) { ++*n_; }
  ~Busy() { --*n_; }
  std::atomic<int>* n_;
};

void TableLoop(int n, int R, int M, int stage, int at, std::vector<int>* written, std::vector<int>* completed, std::atomic<int>* live) {
  auto nap = [](long id, int who) {
    if ((id + who) % 5 == 0) std::this_thread::sleep_for(std::chrono::microseconds(100 + 40 * who));
  };
  xv::BoundedQueue<LoopItem> plans(2 * R + 3), queue(2 * R + 3);
  xv::BoundedQueue<char> credits(2 * R + 2);
  xv::ReorderBuffer<LoopItem> filled;
  xv::FirstError reader_error;
  for (int i = 0; i < 2 * R + 2; ++i) credits.Push(0);
  auto stop_readers = [&] {
    plans.Cancel();
    queue.Cancel();
    credits.Cancel();
  };
  xv::ThreadGroup readers(stop_readers);
  readers.Start("st-index", [&] {
    Busy busy(live);
    for (int id = 0; id <= n; ++id) {
      char credit;
      LoopItem it;
      it.seq = id;
      it.last = id == n;
      if (!credits.Pop(&credit) || !plans.Push(std::move(it))) return;
    }
    plans.Close();
  });
  for (int r = 0; r < R; ++r)
    readers.Start("st-read", [&, r] {
      Busy busy(live);
      LoopItem it;
      while (plans.Pop(&it)) {
        try {
          if (stage == 1 && it.seq == at) throw std::runtime_error("produce " + std::to_string(it.seq));
          if (!it.last) it.payload.assign(16 + it.seq % 5, (int)it.seq);
        } catch (...) {
          reader_error.Set(std::current_exception());
          it.bad = true;
        }
        nap(it.seq, r);
        filled.Put(it.seq, std::move(it), [&](LoopItem&& next) { queue.Push(std::move(next)); });
      }
    });

  xv::ReorderBuffer<LoopOut> done;
  xv::FirstError fatal([&] { done.Interrupt(); });
  std::mutex completed_mu;
  auto process = [&](LoopItem&& it, int who) {
    LoopOut o;
    if (!it.bad && !it.last && !fatal.is_set()) {
      try {
        if (stage == 2 && it.seq == at) throw std::runtime_error("work " + std::to_string(it.seq));
        for (int v : it.payload) o.worked += v;
        o.id = (int)it.seq;
        nap(it.seq, who + 1);
        std::lock_guard<std::mutex> lk(completed_mu);
        completed->push_back(o.id);
      } catch (...) {
        fatal.Set(std::current_exception());
        o = LoopOut();
      }
    }
    done.Put(it.seq, std::move(o));
  };
  std::vector<std::unique_ptr<xv::BoundedQueue<LoopItem>>> inbox;
  xv::ThreadGroup workers([&] {
    for (auto& q : inbox) q->Close();
  });
  for (int e = 0; M > 1 && e < M; ++e) {
    inbox.emplace_back(new xv::BoundedQueue<LoopItem>(2));
    workers.Start(nullptr, [&, e, q = inbox[e].get()] {
      Busy busy(live);
      LoopItem it;
      while (q->Pop(&it)) process(std::move(it), e);
    });
  }
  auto write = [&](const LoopOut& o) {
    if (o.id < 0) return;
    if (stage == 3 && o.id == at) throw std::runtime_error("consume " + std::to_string(o.id));
    Expect(o.worked == (long)o.id * (16 + o.id % 5), "item " + std::to_string(o.id) + " did not pass a consumer");
    written->push_back(o.id);
  };
  long g = 0;
  LoopItem it;
  LoopOut o;
  while (queue.Pop(&it)) {
    const bool last = it.last;
    if (!last) credits.Push(0);   // one more item may be planned
    if (M == 1) process(std::move(it), 0);
    else inbox[g % M]->Push(std::move(it));
    ++g;
    while (done.TakeNext(&o)) write(o);
    if (last) break;
  }
  if (M > 1) {
    for (auto& q : inbox) q->Close();
    while (done.next() < g && done.WaitNext(&o)) write(o);
    workers.Join();
  }
  while (done.TakeAny(&o)) write(o);
  stop_readers();
  readers.Join();
  if (fatal.is_set()) std::rethrow_exception(fatal.get());
  if (reader_error.is_set()) std::rethrow_exception(reader_error.get());
}

void RunTableLoop(int n, int R, int M, int stage, int at) {
  const std::string tag = "table loop n=" + std::to_string(n) + " R=" + std::to_string(R) + " M=" + std::to_string(M) + " stage=" + std::to_string(stage) +
                          " at=" + std::to_string(at);
  std::vector<int> written, completed;
  std::atomic<int> live(0);
  std::string what;
  try {
    TableLoop(n, R, M, stage, at, &written, &completed, &live);
  } catch (const std::runtime_error& e) {
    what = e.what();
  }
  Expect(live.load() == 0, tag + ": a thread was still running when the loop returned");
  for (size_t i = 1; i < written.size(); ++i) Expect(written[i] > written[i - 1], tag + ": item " + std::to_string(written[i]) + " written out of order or twice");
  const char* names[] = {"", "produce ", "work ", "consume "};
  Expect(what == (stage ? names[stage] + std::to_string(at) : std::string()), tag + ": expected the stage's exception, got '" + what + "'");
  size_t before = 0;   // items in front of the failing one that were written
  while (before < written.size() && written[before] == (int)before) ++before;
  if (stage == 0) Expect((int)before == n && (int)written.size() == n, tag + ": " + std::to_string(written.size()) + " items written");
  if (stage == 1) Expect((int)before == at && (int)written.size() == n - 1, tag + ": not everything but the unreadable item was written");
  std::sort(completed.begin(), completed.end());
  if (stage == 2)   // what a consumer completed, before the failure or beside it, is written; the failing item is not
    Expect(written == completed && (int)before >= (M == 1 ? at : 0) && std::find(written.begin(), written.end(), at) == written.end(),
           tag + ": " + std::to_string(written.size()) + " items written, " + std::to_string(completed.size()) + " completed");
  if (stage == 3) Expect((int)before == at && (int)written.size() == at, tag + ": the writer did not stop at the failing item");
}

}  // namespace

int main() {
  const int n = 300;
  for (int R : {1, 4})
    for (int M : {1, 3}) {
      RunTableLoop(n, R, M, 0, -1);
      RunTableLoop(0, R, M, 0, -1);
      for (int stage = 1; stage <= 3; ++stage)
        for (int at : {0, 149, n - 1}) RunTableLoop(n, R, M, stage, at);
    }
  for (int slow = 0; slow <= 3; ++slow) Run(n, 0, -1, slow);
  Run(0, 0, -1, 0);   // an empty stream
  Run(1, 0, -1, 0);
  for (int stage = 1; stage <= 3; ++stage)
    for (int at : {0, 1, 149, n - 1})
      for (int slow = 0; slow <= 3; ++slow) Run(n, stage, at, slow);
  Run(n, 1, n, 0);   // the reader fails where the stream would have ended: everything before it is written
  if (g_failures) {
    fprintf(stderr, "stage_pipeline selftest: %d check(s) failed\n", g_failures.load());
    return 1;
  }
  printf("stage_pipeline selftest: ok\n");
  return 0;
}
