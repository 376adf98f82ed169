// Shared by the tools that read a feature table and a side table of one value per utterance - a Gaussian selection or a
// posterior - side by side (ubm_tools_main.cc, gmm_classify_tools_main.cc, gmm_acc_tool.h, post_tools_main.cc, ivex_tools_main.cc,
// ivex_train_tools_main.cc).  Host only.
#pragma once
#include <string>
#include <unordered_map>
#include <utility>

#include "cli.h"
#include "kio.h"

namespace xv {

// The value of a key: a table that promised sorted keys (s) is merged front to back, any other is loaded.  noun: what the
// warning about an entry that cannot be read calls the values.
template <class T>
class KeyedLookup {
 public:
  KeyedLookup(const std::string& rspecifier, const char* noun) : reader_(rspecifier, false, /*permissive_skips=*/true), noun_(noun) {
    if (reader_.sorted()) return;
    std::string key;
    T v;
    while (Read(&key, &v)) all_.emplace(key, std::move(v));
  }
  bool Find(const std::string& key, T* out) {
    if (!reader_.sorted()) {
      auto it = all_.find(key);
      if (it == all_.end()) return false;
      *out = it->second;
      return true;
    }
    for (;;) {
      if (!held_) {
        if (eof_ || !Read(&held_key_, &held_v_)) {
          eof_ = true;
          return false;
        }
        held_ = true;
      }
      const int c = held_key_.compare(key);
      if (c > 0) return false;   // the table is past the key
      held_ = false;
      if (c == 0) {
        *out = std::move(held_v_);
        return true;
      }
    }
  }

 private:
  // the next entry that can be read; false at the end of the table
  bool Read(std::string* key, T* v) {
    for (;;) {
      std::string err;
      if (!reader_.Next(key, v, &err)) return false;
      if (err.empty()) return true;
      XWARN("Failed to read the " << noun_ << " of " << *key << ": " << err);
    }
  }
  SequentialTableReader<T> reader_;
  const char* noun_;
  std::unordered_map<std::string, T> all_;
  bool held_ = false, eof_ = false;
  std::string held_key_;
  T held_v_;
};

struct GselectLookup : KeyedLookup<IntVecVec> {
  explicit GselectLookup(const std::string& rspecifier) : KeyedLookup(rspecifier, "Gaussian selection") {}
};
struct PosteriorLookup : KeyedLookup<Posterior> {
  explicit PosteriorLookup(const std::string& rspecifier) : KeyedLookup(rspecifier, "posterior") {}
};

}  // namespace xv
