// Shared by the tools that join a feature table with a table of Gaussian selections (ubm_tools_main.cc, ubm_train_tools_main.cc).
#pragma once
#include <string>
#include <unordered_map>
#include <utility>

#include "cli.h"
#include "kio.h"

namespace xv {

// The Gaussian selection of a key: a table that promised sorted keys (s) is merged front to back, any other is loaded.
class GselectLookup {
 public:
  explicit GselectLookup(const std::string& rspecifier) : reader_(rspecifier) {
    if (reader_.sorted()) return;
    std::string key, err;
    xv::IntVecVec v;
    while (reader_.Next(&key, &v, &err)) {
      if (!err.empty()) XWARN("Failed to read the Gaussian selection of " << key << ": " << err);
      else all_.emplace(key, std::move(v));
    }
  }
  bool Find(const std::string& key, xv::IntVecVec* out) {
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
          XWARN("Failed to read the Gaussian selection of " << held_key_ << ": " << err);
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
  xv::SequentialGselectReader reader_;
  std::unordered_map<std::string, xv::IntVecVec> all_;
  bool held_ = false, eof_ = false;
  std::string held_key_;
  xv::IntVecVec held_v_;
};

}  // namespace xv
