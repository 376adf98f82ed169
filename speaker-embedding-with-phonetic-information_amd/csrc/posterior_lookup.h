// The posterior of a key, for the tools that read a feature table and a posterior table side by side (ivector-extract,
// ivector-extractor-acc-stats).  Host only.
#pragma once
#include <string>
#include <unordered_map>
#include <utility>

#include "cli.h"
#include "kio.h"

namespace xv {

// The posterior of a key: a table that promised sorted keys (s) is merged front to back, any other is loaded.
class PosteriorLookup {
 public:
  explicit PosteriorLookup(const std::string& rspecifier) : reader_(rspecifier) {
    if (reader_.sorted()) return;
    std::string key, err;
    Posterior v;
    while (reader_.Next(&key, &v, &err)) {
      if (!err.empty()) XWARN("Failed to read the posterior of " << key << ": " << err);
      else all_.emplace(key, std::move(v));
    }
  }
  bool Find(const std::string& key, Posterior* out) {
    if (!reader_.sorted()) {
      auto it = all_.find(key);
      if (it == all_.end()) return false;
      *out = it->second;
      return true;
    }
    for (;;) {
      if (!held_) {
        std::string err;
        if (eof_ || !reader_.Next(&held_key_, &held_v_, &err)) {
          eof_ = true;
          return false;
        }
        if (!err.empty()) {
          XWARN("Failed to read the posterior of " << held_key_ << ": " << err);
          continue;
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
  SequentialPosteriorReader reader_;
  std::unordered_map<std::string, Posterior> all_;
  bool held_ = false, eof_ = false;
  std::string held_key_;
  Posterior held_v_;
};

}  // namespace xv
