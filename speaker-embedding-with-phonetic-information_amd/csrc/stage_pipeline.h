// The threading of the table loops, and nothing else: no device, no table, stages as functions, so that all of it can be run -
// and put under a sanitizer - without either (stage_pipeline_selftest_main.cc).
//
//   BoundedQueue    first in, first out, at most `depth` items; Close() ends the stream, Cancel() releases every waiter.
//   ReorderBuffer   items filed by number in any order leave in the order of their numbers.
//   FirstError      the first failure of a job, whoever meets it; setting it can wake a waiter.
//   ThreadGroup     threads that are released and joined when the group goes, however the scope is left.
//   RunThreeStages  read-ahead, work and write-behind over a stream of items (nnet3-compute's loop, table_compute.cc).
//
// RunThreeStages: while the device works on one batch, the next one is being read and the previous one written.
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
#include <map>
#include <mutex>
#include <pthread.h>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

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

// Items filed under their numbers in any order (every number once) leave in the order of the numbers, starting at 0.
template <class T>
class ReorderBuffer {
 public:
  void Put(long seq, T&& item) {
    Put(seq, std::move(item), nullptr);
  }
  // ... and hands on what is now next in sequence: sink(T&&) runs under the buffer's lock, so that what two threads file
  // leaves in one order; it must not wait for whoever files.
  template <class Sink>
  void Put(long seq, T&& item, Sink sink) {
    std::lock_guard<std::mutex> lk(mu_);
    items_.emplace(seq, std::move(item));
    if constexpr (!std::is_same<Sink, std::nullptr_t>::value) {
      T next;
      while (Take(false, &next)) sink(std::move(next));
    }
    cv_.notify_all();
  }
  // The item that is next in sequence, waited for.  false: it is not there and Interrupt() was called.
  bool WaitNext(T* out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return interrupted_ || items_.count(next_); });
    return Take(false, out);
  }
  bool TakeNext(T* out) {   // the same without waiting
    std::lock_guard<std::mutex> lk(mu_);
    return Take(false, out);
  }
  // The lowest number that is there, gaps included: after a failure, what was finished is still handed on.
  bool TakeAny(T* out) {
    std::lock_guard<std::mutex> lk(mu_);
    return Take(true, out);
  }
  void Interrupt() {
    std::lock_guard<std::mutex> lk(mu_);
    interrupted_ = true;
    cv_.notify_all();
  }
  long next() {   // the number that leaves next = how many have left when there were no gaps
    std::lock_guard<std::mutex> lk(mu_);
    return next_;
  }

 private:
  bool Take(bool any, T* out) {
    auto it = items_.begin();
    if (it == items_.end() || (!any && it->first != next_)) return false;
    next_ = it->first + 1;
    *out = std::move(it->second);
    items_.erase(it);
    return true;
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::map<long, T> items_;
  long next_ = 0;
  bool interrupted_ = false;
};

// The first failure of a job.  `wake` (optional) runs on every Set, on the setter's thread: it releases whoever waits for
// something the failure may keep from coming (ReorderBuffer::Interrupt, BoundedQueue::Cancel).
class FirstError {
 public:
  explicit FirstError(std::function<void()> wake = nullptr) : wake_(std::move(wake)) {}
  void Set(std::exception_ptr e) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (!first_) first_ = e;
    }
    if (wake_) wake_();
  }
  void Set(const std::string& what) { Set(std::make_exception_ptr(std::runtime_error(what))); }
  std::exception_ptr get() const {
    std::lock_guard<std::mutex> lk(mu_);
    return first_;
  }
  bool is_set() const { return get() != nullptr; }
  std::string what() const {   // "": none
    const std::exception_ptr e = get();
    if (!e) return std::string();
    try {
      std::rethrow_exception(e);
    } catch (const std::exception& ex) {
      return ex.what();
    } catch (...) {
      return "unknown error";
    }
  }

 private:
  const std::function<void()> wake_;
  mutable std::mutex mu_;
  std::exception_ptr first_;
};

// Threads that do not outlive their scope: the destructor calls `release` (which must make every body return: close or cancel
// what the bodies wait for) and joins.  A joinable std::thread destroyed by unwinding would be std::terminate.  A body must
// not let an exception escape.  name (optional): what the thread is called in /proc and in a profile.
class ThreadGroup {
 public:
  explicit ThreadGroup(std::function<void()> release = nullptr) : release_(std::move(release)) {}
  ThreadGroup(const ThreadGroup&) = delete;
  ThreadGroup& operator=(const ThreadGroup&) = delete;
  ~ThreadGroup() {
    if (release_) release_();
    Join();
  }
  void Start(const char* name, std::function<void()> body) {
    threads_.emplace_back([name, body] {
      if (name) (void)pthread_setname_np(pthread_self(), name);
      body();
    });
  }
  void Join() {
    for (std::thread& t : threads_)
      if (t.joinable()) t.join();
    threads_.clear();
  }

 private:
  const std::function<void()> release_;
  std::vector<std::thread> threads_;
};

template <class Item>
void RunThreeStages(const std::function<bool(Item*)>& produce, const std::function<void(Item*)>& work,
                    const std::function<void(Item*)>& consume, size_t depth = 2) {
  BoundedQueue<Item> ahead(depth), behind(depth);
  FirstError error;
  auto fail = [&] {
    error.Set(std::current_exception());
    ahead.Cancel();
    behind.Cancel();
  };
  {
    ThreadGroup threads;
    threads.Start(nullptr, [&] {
      try {
        for (;;) {
          Item it;
          if (!produce(&it) || !ahead.Push(std::move(it))) break;
        }
      } catch (...) {
        error.Set(std::current_exception());   // what was produced before the failure is still worked on and consumed
      }
      ahead.Close();
    });
    threads.Start(nullptr, [&] {
      try {
        Item it;
        while (behind.Pop(&it)) consume(&it);
      } catch (...) {
        fail();
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
      fail();
    }
  }
  if (error.is_set()) std::rethrow_exception(error.get());
}

}  // namespace xv

