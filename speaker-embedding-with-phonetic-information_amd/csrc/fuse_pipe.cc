// See fuse_pipe.h.
#include "fuse_pipe.h"

#include <stdlib.h>

#include <algorithm>
#include <sstream>
#include <vector>

namespace xv {

namespace {

std::string Basename(const std::string& p) {
  const size_t s = p.rfind('/');
  return s == std::string::npos ? p : p.substr(s + 1);
}

bool ParseBoolValue(const std::string& v, bool* out) {
  if (v == "true" || v == "t" || v == "1") {
    *out = true;
    return true;
  }
  if (v == "false" || v == "f" || v == "0") {
    *out = false;
    return true;
  }
  return false;
}

bool ParseIntValue(const std::string& v, long lowest, int* out) {
  if (v.empty()) return false;
  char* end = nullptr;
  const long x = strtol(v.c_str(), &end, 10);
  if (*end || x < lowest || x > 1000000) return false;
  *out = (int)x;
  return true;
}

std::vector<std::string> Words(const std::string& s) {
  std::istringstream in(s);
  std::vector<std::string> w;
  std::string t;
  while (in >> t) w.push_back(t);
  return w;
}

// The stages of "ark[,letters]:stage | stage |" (the text between the bars), or false: a character a shell would interpret beyond
// words and the bar disqualifies the string - it is then a command line, not one of the pipelines here - and so does a missing
// prefix or a missing last bar.  option_letters: Kaldi's rspecifier options may stand between "ark" and the colon.
bool PipelineStages(const std::string& rspecifier, bool option_letters, std::vector<std::string>* stages) {
  for (char c : rspecifier)
    if (c == '\'' || c == '"' || c == '\\' || c == '`' || c == '$' || c == ';' || c == '&' || c == '<' || c == '>' || c == '(' ||
        c == ')' || c == '*' || c == '?' || c == '~' || c == '\n')
      return false;
  std::string s = rspecifier;
  while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
  if (s.compare(0, 3, "ark") != 0 || s.back() != '|') return false;
  const size_t colon = s.find(':');
  if (colon == std::string::npos || (!option_letters && colon != 3)) return false;
  for (size_t a = 3; a < colon;) {   // ",s,cs": every letter group one Kaldi knows
    if (s[a] != ',') return false;
    const size_t b = std::min(s.find(',', a + 1), colon);
    const std::string o = s.substr(a + 1, b - a - 1);
    if (o != "s" && o != "cs" && o != "o" && o != "p" && o != "ns" && o != "ncs" && o != "no" && o != "np" && o != "bg") return false;
    a = b;
  }
  s = s.substr(colon + 1, s.size() - colon - 2);
  for (size_t a = 0;;) {
    const size_t b = s.find('|', a);
    stages->push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
    if (b == std::string::npos) break;
    a = b + 1;
  }
  return true;
}

// a table in a file: "scp:<file>" or "ark:<file>", with the option letters Kaldi allows in front of the colon
bool IsFileTable(const std::string& w, const char* only_kind = nullptr) {
  if (w.compare(0, 2, "--") == 0) return false;
  const size_t colon = w.find(':');
  if (colon == std::string::npos || colon + 1 >= w.size()) return false;
  const std::string kind = w.substr(0, w.find_first_of(",:"));
  if (only_kind ? kind != only_kind : (kind != "scp" && kind != "ark")) return false;
  const std::string target = w.substr(colon + 1);
  return target != "-" && target.back() != '|';
}

// "--name=value" with underscores read as dashes; false: not of that form
bool SplitOption(const std::string& w, std::string* name, std::string* value) {
  const size_t eq = w.find('=');
  if (w.compare(0, 2, "--") != 0 || eq == std::string::npos) return false;
  *name = w.substr(2, eq - 2);
  for (char& c : *name)
    if (c == '_') c = '-';
  *value = w.substr(eq + 1);
  return true;
}

// the optional second stage: "select-voiced-frames ark:- <vad table in a file> ark:-"
bool SelectStage(const std::string& stage, std::string* vad) {
  const std::vector<std::string> w = Words(stage);
  if (w.size() != 4 || Basename(w[0]) != "select-voiced-frames" || w[1] != "ark:-" || w[3] != "ark:-" || !IsFileTable(w[2])) return false;
  *vad = w[2];
  return true;
}

}  // namespace

bool RecognizeFeaturePipeline(const std::string& rspecifier, FusedPipeline* out) {
  std::vector<std::string> stages;
  if (!PipelineStages(rspecifier, false, &stages) || stages.size() > 2) return false;
  FusedPipeline p;
  {
    const std::vector<std::string> w = Words(stages[0]);
    if (w.size() < 3 || Basename(w[0]) != "apply-cmvn-sliding") return false;
    std::vector<std::string> pos;
    for (size_t i = 1; i < w.size(); ++i) {
      if (w[i].compare(0, 2, "--") != 0) {
        pos.push_back(w[i]);
        continue;
      }
      std::string name, value;
      if (!SplitOption(w[i], &name, &value)) return false;
      bool b = false;
      if (name == "norm-vars") {
        if (!ParseBoolValue(value, &b) || b) return false;        // variance normalisation: not what the device front-end does
      } else if (name == "center") {
        if (!ParseBoolValue(value, &p.center)) return false;
      } else if (name == "cmn-window") {
        if (!ParseIntValue(value, 1, &p.cmn_window)) return false;
      } else if (name == "min-cmn-window") {
        // the tool takes this value as typed, zero and below included (no minimum then: max(t + 1, M) is t + 1), and so does the
        // device: the fused job and the command it names run the same windows
        if (!ParseIntValue(value, -1000000, &p.min_cmn_window)) return false;
      } else {
        return false;                                             // --max-warnings, --verbose, --config ...: run the command
      }
    }
    if (pos.size() != 2 || pos[1] != "ark:-" || !IsFileTable(pos[0])) return false;
    p.feats_rspecifier = pos[0];
  }
  if (stages.size() == 2 && !SelectStage(stages[1], &p.vad_rspecifier)) return false;
  *out = p;
  return true;
}

bool RecognizeCmvnPipeline(const std::string& rspecifier, FusedCmvnPipeline* out) {
  std::vector<std::string> stages;
  if (!PipelineStages(rspecifier, true, &stages) || stages.size() > 2) return false;
  FusedCmvnPipeline p;
  {
    const std::vector<std::string> w = Words(stages[0]);
    if (w.size() < 4 || Basename(w[0]) != "apply-cmvn") return false;
    std::vector<std::string> pos;
    for (size_t i = 1; i < w.size(); ++i) {
      if (w[i].compare(0, 2, "--") != 0) {
        pos.push_back(w[i]);
        continue;
      }
      std::string name, value;
      if (!pos.empty() || !SplitOption(w[i], &name, &value)) return false;   // the tool takes its options in front
      if (name == "norm-means") {
        if (!ParseBoolValue(value, &p.norm_means)) return false;
      } else if (name == "norm-vars") {
        if (!ParseBoolValue(value, &p.norm_vars)) return false;
      } else if (name == "utt2spk") {
        if (!IsFileTable(value, "ark")) return false;
        p.utt2spk_rspecifier = value;
      } else {
        return false;                                               // --skip-dims, --reverse, --config, --verbose ...: run the command
      }
    }
    if (pos.size() != 3 || pos[2] != "ark:-" || !IsFileTable(pos[1])) return false;
    p.stats_is_table = IsFileTable(pos[0]);
    // anything else in the first position is a file that holds the one global matrix - if it can be a file's name at all
    if (!p.stats_is_table && (pos[0] == "-" || pos[0].find(':') != std::string::npos)) return false;
    p.stats_rxfilename = pos[0];
    p.feats_rspecifier = pos[1];
  }
  if (stages.size() == 2 && !SelectStage(stages[1], &p.vad_rspecifier)) return false;
  *out = p;
  return true;
}

std::string DescribeFusedCmvn(const FusedCmvnPipeline& p) {
  std::ostringstream o;
  o << "stats=" << p.stats_rxfilename << "\nstats-is-table=" << (p.stats_is_table ? "true" : "false") << "\nfeats=" << p.feats_rspecifier
    << "\nvad=" << p.vad_rspecifier << "\nutt2spk=" << p.utt2spk_rspecifier << "\nnorm-means=" << (p.norm_means ? "true" : "false")
    << "\nnorm-vars=" << (p.norm_vars ? "true" : "false") << "\n";
  return o.str();
}

}  // namespace xv
