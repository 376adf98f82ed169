// Three stages over a stream of items, in order: read-ahead, work and write-behind, each on a thread of its own with a bounded
// queue between neighbours.  What nnet3-compute's table loop is made of (table_extract.cc RunTableCompute): while the device
// works on one batch, the next one is being read and the previous one written.  Nothing here names the device or a table: the
// stages are three functions, so the threading can be run - and put under a sanitizer - without either
// (stage_pipeline_selftest_main.cc).
//
//   produce(Item*) -> bool   fills the next item; false: the stream has ended (the item is not used).  Reader thread.
//   work(Item*)              the middle stage, on the CALLING thread: the one that owns whatever must stay on one thread.
//   consume(Item*)           takes the finished item.  Writer thread.
//
// Items leave in the order they were produced: each queue is first in, first out, and each stage is one thread.  At most `depth`
// items wait in each queue, so a fast reader cannot run ahead of a slow device by more than that.  An exception in work or
// consume stops the other two stages at their next queue operation (an item that is being worked on is finished first, nothing
// new is started).  An exception in produce ends the stream there: the items produced before it are still worked on and
// consumed - a table that turns out to be corrupt half way leaves everything in front of the bad entry written.  Either way all
// threads are joined and the FIRST exception is rethrown on the calling thread.
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

namespace xv {

template <class T>
class BoundedQueue {
 public:
  explicit BoundedQueue(size_t depth) : depth_(depth ? depth : 1) {}
  // false: the pipeline was cancelled (the item is dropped)
  bool Push(T&& v) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return cancelled_ || q_.size() < depth_; });
    if (cancelled_) return false;
    q_.push_back(std::move(v));
    cv_.notify_all();
    return true;
  }
  // false: nothing more will come (closed and drained, or cancelled)
  bool Pop(T* out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return cancelled_ || closed_ || !q_.empty(); });
    if (cancelled_ || q_.empty()) return false;
    *out = std::move(q_.front());
    q_.pop_front();
    cv_.notify_all();
    return true;
  }
  void Close() { Set(&closed_); }     // the producer is done: Pop drains what is queued, then returns false
  void Cancel() { Set(&cancelled_); } // a stage failed: every waiter returns false at once

 private:
  void Set(bool* flag) {
    std::lock_guard<std::mutex> lk(mu_);
    *flag = true;
    cv_.notify_all();
  }
  const size_t depth_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<T> q_;
  bool closed_ = false, cancelled_ = false;
};

template <class Item>
void RunThreeStages(const std::function<bool(Item*)>& produce, const std::function<void(Item*)>& work,
                    const std::function<void(Item*)>& consume, size_t depth = 2) {
  BoundedQueue<Item> ahead(depth), behind(depth);
  std::mutex err_mu;
  std::exception_ptr first;
  auto fail = [&](std::exception_ptr e) {
    {
      std::lock_guard<std::mutex> lk(err_mu);
      if (!first) first = e;
    }
    ahead.Cancel();
    behind.Cancel();
  };
  std::thread reader([&] {
    try {
      for (;;) {
        Item it;
        if (!produce(&it) || !ahead.Push(std::move(it))) break;
      }
      ahead.Close();
    } catch (...) {
      {
        std::lock_guard<std::mutex> lk(err_mu);
        if (!first) first = std::current_exception();
      }
      ahead.Close();   // what was produced before the failure is still worked on and consumed
    }
  });
  std::thread writer([&] {
    try {
      Item it;
      while (behind.Pop(&it)) consume(&it);
    } catch (...) {
      fail(std::current_exception());
    }
  });
  try {
    Item it;
    while (ahead.Pop(&it)) {
      work(&it);
      if (!behind.Push(std::move(it))) break;
    }
    behind.Close();
  } catch (...) {
    fail(std::current_exception());
  }
  reader.join();
  writer.join();
  if (first) std::rethrow_exception(first);
}

}  // namespace xv
