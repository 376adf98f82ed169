// Stand-alone check of stage_pipeline.h, meant to be built with a sanitizer (make sanitize-pipeline: once with
// -fsanitize=thread, once with -fsanitize=address,undefined) and run on a machine without a GPU: a few hundred items through
// the three stages with stages of uneven speed, then the same with a stage that throws at a chosen item, for every stage and
// for the first, a middle and the last item.  Checks: every item arrives, in order, with what each stage did to it; a throw
// comes back out of RunThreeStages as that exception, after both threads were joined (the function returned), nothing at or
// behind the failing item was consumed, and everything in front of an item the reader failed on was.  Exit status 0 and "stage_pipeline selftest: ok" when all of it holds.
#include <stdio.h>

#include <atomic>
#include <chrono>
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

}  // namespace

int main() {
  const int n = 300;
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
