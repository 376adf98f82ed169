// See fuse_wav.h.
#include "fuse_wav.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <sstream>
#include <tuple>

#include "kio.h"
#include "reverb.h"
#include "wave.h"

namespace xv {
namespace {

std::string Basename(const std::string& p) {
  const size_t s = p.rfind('/');
  return s == std::string::npos ? p : p.substr(s + 1);
}

std::string Trim(const std::string& s) {
  const size_t f = s.find_first_not_of(" \t");
  if (f == std::string::npos) return std::string();
  return s.substr(f, s.find_last_not_of(" \t") - f + 1);
}

// Positions of the '|' outside quotes; false for unbalanced quotes.
bool TopLevelPipes(const std::string& s, std::vector<size_t>* pipes) {
  char q = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    const char c = s[i];
    if (q) {
      if (c == q) q = 0;
    } else if (c == '\'' || c == '"') {
      q = c;
    } else if (c == '|') {
      pipes->push_back(i);
    }
  }
  return q == 0;
}

// Words of one stage as a shell would form them from plain text and quotes; false when the stage holds anything a shell would
// expand or interpret beyond that.
bool ShellWords(const std::string& s, std::vector<std::string>* words) {
  std::string cur;
  bool have = false;
  char q = 0;
  for (char c : s) {
    if (c == '\\' || c == '`' || c == '$' || c == '\n') return false;
    if (q) {
      if (c == q) q = 0;
      else cur.push_back(c);
      continue;
    }
    if (c == '\'' || c == '"') {
      q = c;
      have = true;
    } else if (c == ' ' || c == '\t') {
      if (have) words->push_back(cur);
      cur.clear();
      have = false;
    } else if (c == ';' || c == '&' || c == '<' || c == '>' || c == '(' || c == ')' || c == '*' || c == '?' || c == '~' || c == '#' ||
               c == '{' || c == '}' || c == '[' || c == ']' || c == '!') {
      return false;
    } else {
      cur.push_back(c);
      have = true;
    }
  }
  if (q) return false;
  if (have) words->push_back(cur);
  return true;
}

bool ParseBool(const std::string& v, int32_t* out) {
  if (v == "true" || v == "t" || v == "1" || v.empty()) *out = 1;
  else if (v == "false" || v == "f" || v == "0") *out = 0;
  else return false;
  return true;
}
bool ParseFloat(const std::string& v, float* out) {
  char* end = nullptr;
  const double d = strtod(v.c_str(), &end);
  if (v.empty() || !end || *end) return false;
  *out = (float)d;
  return true;
}
bool ParseInt(const std::string& v, int32_t* out) {
  char* end = nullptr;
  const long d = strtol(v.c_str(), &end, 10);
  if (v.empty() || !end || *end) return false;
  *out = (int32_t)d;
  return true;
}

std::vector<std::string> SplitCommas(const std::string& s) {
  std::vector<std::string> out;
  size_t a = 0;
  while (a <= s.size()) {
    const size_t b = s.find(',', a);
    const std::string e = Trim(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
    if (!e.empty()) out.push_back(e);
    if (b == std::string::npos) break;
    a = b + 1;
  }
  return out;
}

bool Recognize(const std::string& rx, bool nested, FusedWav* out) {
  const std::string s = Trim(rx);
  if (s.empty() || s.back() != '|') return false;
  std::vector<size_t> pipes;
  if (!TopLevelPipes(s, &pipes)) return false;
  if (pipes.empty() || pipes.back() != s.size() - 1) return false;   // a quoted last '|' is not a pipe
  const size_t begin = pipes.size() >= 2 ? pipes[pipes.size() - 2] + 1 : 0;
  const std::string stage = s.substr(begin, s.size() - 1 - begin);
  const std::string source = Trim(s.substr(0, begin));               // "" or "stage | ... |"
  std::vector<std::string> w;
  if (!ShellWords(stage, &w) || w.empty() || Basename(w[0]) != "wav-reverberate") return false;
  FusedWav p;
  p.opts = ReverbDefaults();
  std::string additive, snrs, starts;
  std::vector<std::string> pos;
  for (size_t i = 1; i < w.size(); ++i) {
    if (w[i].compare(0, 2, "--") != 0 || !pos.empty()) {
      pos.push_back(w[i]);
      continue;
    }
    const size_t eq = w[i].find('=');
    const std::string name = w[i].substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
    const std::string value = eq == std::string::npos ? std::string() : w[i].substr(eq + 1);
    bool ok;
    if (name == "impulse-response") { p.impulse_response = value; ok = !value.empty(); }
    else if (name == "duration") ok = ParseFloat(value, &p.opts.duration);
    else if (nested) ok = false;
    else if (name == "additive-signals") { additive = value; ok = true; }
    else if (name == "snrs") { snrs = value; ok = true; }
    else if (name == "start-times") { starts = value; ok = true; }
    else if (name == "shift-output") ok = ParseBool(value, &p.opts.shift_output);
    else if (name == "normalize-output") ok = ParseBool(value, &p.opts.normalize_output);
    else if (name == "volume") ok = ParseFloat(value, &p.opts.volume);
    else if (name == "input-wave-channel") ok = ParseInt(value, &p.opts.input_wave_channel);
    else if (name == "rir-channel") ok = ParseInt(value, &p.opts.rir_channel);
    else if (name == "noise-channel") ok = ParseInt(value, &p.opts.noise_channel);
    else ok = false;   // --multi-channel-output, --verbose, --config, ...: run the command
    if (!ok) return false;
  }
  if (pos.size() != 2 || pos[1] != "-") return false;
  if (pos[0] == "-") {
    if (source.empty()) return false;
    p.source = source;
  } else {
    if (!source.empty() || pos[0].back() == '|' || pos[0].compare(0, 2, "--") == 0) return false;
    p.source = pos[0];
  }
  if (nested && source.find("wav-reverberate") != std::string::npos) return false;
  if (p.impulse_response.find("wav-reverberate") != std::string::npos) return false;
  if (p.source.find("wav-reverberate") != std::string::npos) return false;   // the tool in front of the tool: a command
  const std::vector<std::string> add = SplitCommas(additive), sn = SplitCommas(snrs), st = SplitCommas(starts);
  for (size_t i = 0; i < add.size(); ++i) {
    FusedWavAdd a;
    if (i < sn.size() && !ParseFloat(sn[i], &a.snr)) return false;
    if (i < st.size() && !ParseFloat(st[i], &a.start)) return false;
    if (add[i].find("wav-reverberate") != std::string::npos) {
      a.nested = true;
      a.inner = std::make_shared<FusedWav>();
      if (!Recognize(add[i], true, a.inner.get())) return false;   // deeper nesting, other options: not this pipeline
    } else {
      a.rx = add[i];
    }
    p.add.push_back(a);
  }
  // unequal counts are the tool's error, not a reason to start it: keep what the lists said
  if (sn.size() != add.size() || st.size() != add.size()) {
    FusedWavAdd bad;
    bad.rx = "\n" + std::to_string(add.size()) + ", " + std::to_string(sn.size()) + ", " + std::to_string(st.size());
    p.add.assign(1, bad);
  }
  *out = p;
  return true;
}

void Describe(const FusedWav& p, const std::string& prefix, std::ostringstream* o) {
  *o << prefix << "source=" << p.source << "\n" << prefix << "impulse-response=" << p.impulse_response << "\n"
     << prefix << "shift-output=" << p.opts.shift_output << "\n" << prefix << "normalize-output=" << p.opts.normalize_output << "\n"
     << prefix << "duration=" << p.opts.duration << "\n" << prefix << "volume=" << p.opts.volume << "\n"
     << prefix << "channels=" << p.opts.input_wave_channel << "," << p.opts.rir_channel << "," << p.opts.noise_channel << "\n";
  for (size_t i = 0; i < p.add.size(); ++i) {
    const std::string a = prefix + "additive[" + std::to_string(i) + "].";
    *o << a << "snr=" << p.add[i].snr << "\n" << a << "start=" << p.add[i].start << "\n";
    if (p.add[i].nested) Describe(*p.add[i].inner, a, o);
    else if (!p.add[i].rx.empty() && p.add[i].rx[0] == '\n') *o << a << "count-mismatch=" << p.add[i].rx.substr(1) << "\n";
    else *o << a << "rx=" << p.add[i].rx << "\n";
  }
}

int ReadChannel(const std::string& rx, int channel, const char* what, std::vector<float>* out) {
  Input in;
  in.Open(rx);
  WaveData w;
  ReadWave(in, &w, true);
  const int st = in.Close();
  if (st != 0 && w.samples.empty()) throw KioError("command of " + rx + " exited with status " + std::to_string(st));
  if (channel < 0 || channel >= w.channels)
    throw KioError(std::string("the ") + what + " " + rx + " has " + std::to_string(w.channels) + " channels but channel " +
                   std::to_string(channel) + " was asked for");
  const size_t n = w.frames();
  out->resize(n);
  for (size_t i = 0; i < n; ++i) (*out)[i] = (float)w.samples[i * (size_t)w.channels + (size_t)channel];
  return w.rate;
}

}  // namespace

bool RecognizeWavPipeline(const std::string& rxfilename, FusedWav* out) { return Recognize(rxfilename, false, out); }

std::string DescribeFusedWav(const FusedWav& p) {
  std::ostringstream o;
  Describe(p, "", &o);
  return o.str();
}

void LoadWavJob(const FusedWav& p, WavJob* job) {
  job->opts = p.opts;
  job->rate = ReadChannel(p.source, p.opts.input_wave_channel, "input", &job->input);
  if (job->input.empty()) throw KioError("the input " + p.source + " has no samples");
  if (!p.impulse_response.empty()) {
    const int r = ReadChannel(p.impulse_response, p.opts.rir_channel, "impulse response", &job->rir);
    if (r != job->rate)
      throw KioError("sampling frequency mismatch: the impulse response " + p.impulse_response + " has " + std::to_string(r) +
                     ", the input " + std::to_string(job->rate));
    if (job->rir.empty()) throw KioError("the impulse response " + p.impulse_response + " has no samples");
  }
  if (p.add.size() == 1 && !p.add[0].nested && !p.add[0].rx.empty() && p.add[0].rx[0] == '\n')
    throw KioError("--additive-signals, --snrs and --start-times must list the same number of elements (" + p.add[0].rx.substr(1) + ")");
  for (const FusedWavAdd& a : p.add) {
    job->add.emplace_back();
    WavJob::Add& A = job->add.back();
    A.snr = a.snr;
    A.start = a.start;
    int r;
    if (a.nested) {
      if (p.opts.noise_channel != 0)
        throw KioError("the additive signal from " + a.inner->source + " has 1 channels but channel " + std::to_string(p.opts.noise_channel) + " was asked for");
      A.nested.reset(new WavJob);
      LoadWavJob(*a.inner, A.nested.get());
      r = A.nested->rate;
      if (A.nested->out_len < 1) throw KioError("the additive signal from " + a.inner->source + " has no samples");
    } else {
      r = ReadChannel(a.rx, p.opts.noise_channel, "additive signal", &A.samples);
      if (A.samples.empty()) throw KioError("the additive signal " + a.rx + " has no samples");
    }
    if (r != job->rate)
      throw KioError("sampling frequency mismatch: the additive signal " + (a.nested ? a.inner->source : a.rx) + " has " +
                     std::to_string(r) + ", the input " + std::to_string(job->rate));
  }
  job->out_len = std::max<int64_t>(0, ReverbOutputLength(p.opts, (float)job->rate, (int64_t)job->input.size(), (int64_t)job->rir.size()));
}

namespace {

void RunLevel(int device, const std::vector<WavJob*>& jobs) {
  typedef std::tuple<int, int32_t, int32_t, float, float> Key;
  std::map<Key, std::vector<WavJob*>> groups;
  for (WavJob* j : jobs) groups[Key(j->rate, j->opts.shift_output, j->opts.normalize_output, j->opts.duration, j->opts.volume)].push_back(j);
  for (auto& g : groups) {
    const std::vector<WavJob*>& js = g.second;
    std::vector<float> samples, rirs, noises, snr, start;
    std::vector<int64_t> off = {0}, rir_off = {0}, noise_off = {0};
    std::vector<int32_t> utt_rir, add_off = {0}, add_noise;
    for (WavJob* j : js) {
      samples.insert(samples.end(), j->input.begin(), j->input.end());
      off.push_back((int64_t)samples.size());
      if (j->rir.empty()) {
        utt_rir.push_back(-1);
      } else {
        utt_rir.push_back((int32_t)rir_off.size() - 1);
        rirs.insert(rirs.end(), j->rir.begin(), j->rir.end());
        rir_off.push_back((int64_t)rirs.size());
      }
      for (const WavJob::Add& a : j->add) {
        add_noise.push_back((int32_t)noise_off.size() - 1);
        noises.insert(noises.end(), a.samples.begin(), a.samples.end());
        noise_off.push_back((int64_t)noises.size());
        snr.push_back(a.snr);
        start.push_back(a.start);
      }
      add_off.push_back((int32_t)add_noise.size());
    }
    ReverbBatch b;
    b.rate = (float)js[0]->rate;
    b.samples = samples.data();
    b.sample_off = off.data();
    b.n_utts = (int)js.size();
    b.rirs = rirs.data();
    b.rir_off = rir_off.data();
    b.n_rirs = (int)rir_off.size() - 1;
    b.utt_rir = b.n_rirs ? utt_rir.data() : nullptr;
    b.noises = noises.data();
    b.noise_off = noise_off.data();
    b.n_noises = (int)noise_off.size() - 1;
    if (b.n_noises) {
      b.utt_add_off = add_off.data();
      b.add_noise = add_noise.data();
      b.add_snr = snr.data();
      b.add_start = start.data();
    }
    int64_t total = 0;
    for (WavJob* j : js) total += j->out_len;
    std::vector<float> out_f((size_t)total + 1);
    std::vector<int16_t> out_q((size_t)total + 1);
    std::vector<int64_t> out_off(js.size() + 1), clipped(js.size());
    Reverberate(device, js[0]->opts, b, out_off.data(), out_f.data(), out_q.data(), clipped.data());
    for (size_t u = 0; u < js.size(); ++u) {
      js[u]->out.assign(out_q.begin() + out_off[u], out_q.begin() + out_off[u + 1]);
      js[u]->clipped = clipped[u];
    }
  }
}

}  // namespace

void RunWavJobs(int device, const std::vector<WavJob*>& jobs) {
  std::vector<WavJob*> inner;
  for (WavJob* j : jobs)
    for (WavJob::Add& a : j->add)
      if (a.nested) inner.push_back(a.nested.get());
  if (!inner.empty()) RunLevel(device, inner);
  for (WavJob* j : jobs)
    for (WavJob::Add& a : j->add)
      if (a.nested) {
        a.samples.assign(a.nested->out.begin(), a.nested->out.end());   // the 16-bit samples the nested tool would have written
        a.nested.reset();
      }
  if (!jobs.empty()) RunLevel(device, jobs);
}

}  // namespace xv
