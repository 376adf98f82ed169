#include "wave.h"

#include <ctype.h>
#include <string.h>

namespace xv {
namespace {

uint32_t Le32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t Le16(const unsigned char* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// n bytes or a KioError that names the file and what was being read
void ReadHeaderBytes(Input& in, void* dst, size_t n, const char* what) {
  if (in.ReadUpTo(dst, n) != n) throw KioError(std::string("WAVE: input ends inside ") + what + " of " + in.Name());
}

void SkipBytes(Input& in, size_t n, const char* what) {
  unsigned char buf[4096];
  while (n > 0) {
    const size_t k = n < sizeof buf ? n : sizeof buf;
    ReadHeaderBytes(in, buf, k, what);
    n -= k;
  }
}

}  // namespace

void ReadWave(Input& in, WaveData* w, bool until_end_ok) {
  unsigned char h[12];
  ReadHeaderBytes(in, h, 12, "the RIFF header");
  if (memcmp(h, "RIFF", 4) != 0 || memcmp(h + 8, "WAVE", 4) != 0)
    throw KioError("WAVE: " + in.Name() + " is not a RIFF/WAVE file");
  bool have_fmt = false;
  int bits = 0, block = 0;
  w->samples.clear();
  for (;;) {
    unsigned char ch[8];
    const size_t got = in.ReadUpTo(ch, 8);
    if (got == 0) throw KioError("WAVE: no data chunk in " + in.Name());
    if (got != 8) throw KioError("WAVE: input ends inside a chunk header of " + in.Name());
    const uint32_t size = Le32(ch + 4);
    if (memcmp(ch, "fmt ", 4) == 0) {
      if (size < 16) throw KioError("WAVE: fmt chunk of " + std::to_string(size) + " bytes in " + in.Name());
      unsigned char f[16];
      ReadHeaderBytes(in, f, 16, "the fmt chunk");
      const int format = Le16(f);
      w->channels = Le16(f + 2);
      w->rate = (int)Le32(f + 4);
      block = Le16(f + 12);
      bits = Le16(f + 14);
      if (format != 1 && format != 0xFFFE)
        throw KioError("WAVE: " + in.Name() + " is not PCM (format tag " + std::to_string(format) + ")");
      if (bits != 16)
        throw KioError("WAVE: " + in.Name() + " has " + std::to_string(bits) + " bits per sample; only 16-bit PCM is read");
      if (w->channels < 1 || w->rate < 1 || block != 2 * w->channels)
        throw KioError("WAVE: inconsistent fmt chunk in " + in.Name());
      SkipBytes(in, (size_t)(size - 16) + (size & 1), "the fmt chunk");
      have_fmt = true;
      continue;
    }
    if (memcmp(ch, "data", 4) != 0) {   // LIST, fact, bext, ...
      SkipBytes(in, (size_t)size + (size & 1), "a chunk in front of the data");
      continue;
    }
    if (!have_fmt) throw KioError("WAVE: data chunk before the fmt chunk in " + in.Name());
    const bool open_ended = size == 0 || size == 0xFFFFFFFFu;
    if (open_ended && !until_end_ok)
      throw KioError("WAVE: data chunk without a length inside an archive: " + in.Name());
    std::vector<int16_t>& s = w->samples;
    size_t bytes = 0;
    if (!open_ended) {
      s.resize(((size_t)size + 1) / 2);
      bytes = in.ReadUpTo(s.data(), size);   // fewer: the stream ended early, take what came
      if (bytes == size && (size & 1)) in.Get();
    } else {
      const size_t step = 1 << 20;
      for (;;) {
        s.resize((bytes + step + 1) / 2);
        const size_t k = in.ReadUpTo((char*)s.data() + bytes, step);
        bytes += k;
        if (k < step) break;
      }
    }
    s.resize(bytes / (size_t)block * (size_t)w->channels);   // whole sample frames only
    return;
  }
}

void SelectChannel(const WaveData& w, int channel, std::vector<int16_t>* out, std::string* warn) {
  int c = channel;
  if (c < 0) {
    c = 0;
    if (w.channels > 1 && warn) *warn = "Channel not specified but you have data with " + std::to_string(w.channels) + " channels; defaulting to zero";
  } else if (c >= w.channels) {
    throw KioError("File with id has " + std::to_string(w.channels) + " channels but you specified channel " + std::to_string(channel));
  }
  const size_t n = w.frames();
  out->resize(n);
  if (w.channels == 1) {
    memcpy(out->data(), w.samples.data(), n * 2);
    return;
  }
  for (size_t i = 0; i < n; ++i) (*out)[i] = w.samples[i * (size_t)w.channels + (size_t)c];
}

void WriteWaveI16(const std::string& wxfilename, int rate, const int16_t* samples, int64_t n) {
  if (n < 0 || rate < 1) throw KioError("WAVE: bad arguments for writing " + wxfilename);
  if ((uint64_t)n * 2 + 36 > 0xFFFFFFFFull) throw KioError("WAVE: too many samples for a RIFF file: " + wxfilename);
  unsigned char h[44];
  auto put32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) h[at + i] = (unsigned char)(v >> (8 * i)); };
  auto put16 = [&](int at, uint32_t v) { h[at] = (unsigned char)v; h[at + 1] = (unsigned char)(v >> 8); };
  memcpy(h, "RIFF", 4);
  put32(4, (uint32_t)(36 + n * 2));
  memcpy(h + 8, "WAVEfmt ", 8);
  put32(16, 16);
  put16(20, 1);
  put16(22, 1);
  put32(24, (uint32_t)rate);
  put32(28, (uint32_t)rate * 2);
  put16(32, 2);
  put16(34, 16);
  memcpy(h + 36, "data", 4);
  put32(40, (uint32_t)(n * 2));
  Output out;
  out.Open(wxfilename);
  out.Write(h, sizeof h);
  if (n) out.Write(samples, (size_t)n * 2);   // the hosts this builds for are little-endian
  const int st = out.Close();
  if (st != 0) throw KioError("WAVE: writing " + wxfilename + " failed (status " + std::to_string(st) + ")");
}

int64_t WriteWave(const std::string& wxfilename, int rate, const float* samples, int64_t n) {
  std::vector<int16_t> q((size_t)(n > 0 ? n : 0));
  int64_t clipped = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float v = samples[i];
    if (v >= 32768.f) {
      q[i] = 32767;
      ++clipped;
    } else if (v <= -32769.f) {
      q[i] = -32768;
      ++clipped;
    } else if (v != v) {
      q[i] = 0;
    } else {
      q[i] = (int16_t)(int)v;
    }
  }
  WriteWaveI16(wxfilename, rate, q.data(), n);
  return clipped;
}

SequentialWaveReader::SequentialWaveReader(const std::string& rspecifier) {
  opts_ = ParseRspecifier(rspecifier);
  in_.Open(opts_.rxfilename);
}

bool SequentialWaveReader::Next(std::string* key, WaveData* w, std::string* error) {
  error->clear();
  key->clear();
  int c;
  if (opts_.is_scp) {
    std::string line;
    for (;;) {
      line.clear();
      while ((c = in_.Get()) >= 0 && c != '\n') line.push_back((char)c);
      size_t b = line.find_first_not_of(" \t\r");
      if (b != std::string::npos) {
        line = line.substr(b);
        break;
      }
      if (c < 0) return false;
    }
    const size_t sp = line.find_first_of(" \t");
    *key = line.substr(0, sp);
    if (sp == std::string::npos) {
      *error = "script line has no rxfilename";
      return true;
    }
    std::string rx = line.substr(sp + 1);
    while (!rx.empty() && (rx.back() == ' ' || rx.back() == '\t' || rx.back() == '\r')) rx.pop_back();
    if (hook_ && hook_(rx, w, error)) return true;
    try {
      Input data;
      data.Open(rx);
      ReadWave(data, w, true);
      const int st = data.Close();
      if (st != 0 && w->samples.empty()) *error = "command of " + rx + " exited with status " + std::to_string(st);
    } catch (const KioError& e) {
      *error = e.what();
    }
    return true;
  }
  while ((c = in_.Peek()) >= 0 && isspace(c)) in_.Get();
  if (c < 0) return false;
  while ((c = in_.Peek()) >= 0 && !isspace(c)) key->push_back((char)in_.Get());
  in_.Get();
  ReadWave(in_, w, false);
  return true;
}

}  // namespace xv
