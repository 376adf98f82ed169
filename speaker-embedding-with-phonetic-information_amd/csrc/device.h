// Device plumbing shared by the stage modules (backend, plda, feat, reverb, compress, cmvn, ubm, ivex): the error check, the
// device selection, a device buffer, an event timer and the work items of a launch.  Host code only; everything runs on the
// null stream.  The extractor's engine keeps its own buffers, lanes and events (engine.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "kio.h"

namespace xv {

struct EngineError : public std::runtime_error {
  explicit EngineError(const std::string& m) : std::runtime_error(m) {}
};

inline void Check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw EngineError(std::string(what) + ": " + hipGetErrorString(e));
}

// Selects `device`.  who_needs completes the sentence of the error without a GPU: "the UBM kernels need", "i-vector extraction
// needs".  Call it after the arguments are checked: an argument error comes first and does not name the device.
inline void UseDevice(int device, const char* who_needs) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
    throw EngineError(std::string("no HIP device available: ") + who_needs + " a gfx950 GPU (there is no CPU path)");
  if (device < 0 || device >= n) throw EngineError("device index out of range");
  Check(hipSetDevice(device), "hipSetDevice");
}

inline int64_t CeilDiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The rows of a batch of matrices: off[0] = 0, off[u + 1] - off[u] rows in matrix u.  Returns the number of rows.
inline int64_t CheckOffsets(const char* who, const int32_t* off, int n) {
  if (n < 0 || !off) throw KioError(std::string(who) + ": bad argument");
  if (off[0] != 0) throw KioError(std::string(who) + ": row offsets must start at 0");
  for (int u = 0; u < n; ++u)
    if (off[u + 1] < off[u]) throw KioError(std::string(who) + ": row offsets must not decrease");
  return off[n];
}

// Device buffer that frees itself.  A request for no bytes allocates 8, so that p is never null after one.
struct DevBuf {
  // what Reserve allocates when it has to grow: the bytes asked for, or a quarter more (a buffer that lives across batches of
  // slowly rising size)
  enum class Growth { kExact, kQuarterMore };
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  explicit DevBuf(Growth g) : growth_(g) {}
  explicit DevBuf(size_t n) { Alloc(n); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  // a fresh allocation of n bytes
  void Alloc(size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = n ? n : 8;
    Check(hipMalloc(&p, cap), "hipMalloc");
  }
  // at least n bytes; what the buffer held is lost when it grows
  void Reserve(size_t n) {
    if (p && n <= cap) return;
    Alloc(growth_ == Growth::kQuarterMore ? n + n / 4 : n);
  }
  void Upload(const void* src, size_t n, const char* what) {
    Reserve(n);
    if (n) Check(hipMemcpy(p, src, n, hipMemcpyHostToDevice), what);
  }
  template <typename T>
  void Upload(const std::vector<T>& v, const char* what) { Upload(v.data(), v.size() * sizeof(T), what); }
  void Download(void* dst, size_t n, const char* what) const {
    if (n) Check(hipMemcpy(dst, p, n, hipMemcpyDeviceToHost), what);
  }
  template <typename T> T* as() const { return (T*)p; }

 private:
  Growth growth_ = Growth::kExact;
};

// Elapsed time between marks on the null stream.  Off (nobody asked for a time): no event is created and nothing is recorded.
//   two marks:   Start(); launches; ms = Stop();          any number of times, each Stop() waits for its own mark
//   many marks:  Mark(); launches; Mark(); ... Mark();    then Span(i), which waits for mark i + 1 only
class EventTimer {
 public:
  explicit EventTimer(bool on, int marks = 2) {
    for (int i = 0; on && i < marks; ++i) {
      hipEvent_t e = nullptr;
      const hipError_t err = hipEventCreate(&e);
      if (err != hipSuccess) {
        Destroy();
        Check(err, "hipEventCreate");
      }
      ev_.push_back(e);
    }
  }
  ~EventTimer() { Destroy(); }
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  void Mark() {
    if (used_ < ev_.size()) Check(hipEventRecord(ev_[used_++], nullptr), "hipEventRecord");
  }
  // ms between mark i and mark i + 1
  float Span(size_t i) {
    float ms = 0.f;
    Check(hipEventSynchronize(ev_[i + 1]), "hipEventSynchronize");
    Check(hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]), "hipEventElapsedTime");
    return ms;
  }
  void Start() {
    used_ = 0;
    Mark();
  }
  // ms since Start(); 0 when off
  float Stop() {
    Mark();
    return ev_.empty() ? 0.f : Span(0);
  }

 private:
  void Destroy() {
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    ev_.clear();
  }
  std::vector<hipEvent_t> ev_;
  size_t used_ = 0;
};

// The loop of every entry point that reports kernel times: pass(r, ms) runs the work once and leaves its n times in ms (zero on
// entry), for r = 0 .. reps.  The first pass warms up; best[i] is the smallest ms[i] of the others.
template <class Pass>
void BestOfReps(int reps, int n, float* best, Pass pass) {
  std::vector<float> ms((size_t)n);
  for (int i = 0; i < n; ++i) best[i] = 0.f;
  for (int r = 0; r <= reps; ++r) {
    ms.assign((size_t)n, 0.f);
    pass(r, ms.data());
    for (int i = 0; i < n; ++i)
      if (r == 1 || (r > 1 && ms[i] < best[i])) best[i] = ms[i];
  }
}

// Work items (unit, block) of one launch: a unit is a matrix or an utterance, and takes as many workgroups as it has blocks.
struct WorkItems {
  std::vector<int32_t> unit, blk;
  DevBuf d_unit, d_blk;
  void Add(int u, int64_t blocks) {
    for (int64_t b = 0; b < blocks; ++b) {
      unit.push_back(u);
      blk.push_back((int32_t)b);
    }
  }
  int size() const { return (int)unit.size(); }
  void Upload() {
    d_unit.Upload(unit, "copy work items");
    d_blk.Upload(blk, "copy work items");
  }
};

}  // namespace xv
