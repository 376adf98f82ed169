// wav-reverberate - drop-in command line for stage 2 of the recipes (egs/sre/v2/run_sre10.sh:92-159; the wav.scp lines that
// steps/data/reverberate_data_dir.py:366 and steps/data/augment_data_dir_new.py:86-116 write):
//   wav-reverberate [options] <wav-in-rxfilename> <wav-out-wxfilename>
// One file in, one file out.  The arithmetic runs on the HIP device through libxvec_hip.so (reverb.h); without a GPU the tool
// fails (exit 255).  Option names, defaults and exit codes follow Kaldi's tool; an impulse response or an additive signal that
// is itself a "cmd |" pipe is opened as an rxfilename, as a command.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "cli.h"
#include "kio.h"
#include "reverb.h"
#include "wave.h"

namespace {

const char* kUsage =
    "Corrupts the wave files supplied via input pipe with the specified\n"
    "room-impulse response (rir_matrix) and additive noise distortions\n"
    "(specified by corresponding files).\n"
    "Usage:  wav-reverberate [options...] <wav-in-rxfilename> <wav-out-wxfilename>\n"
    "e.g.\n"
    "wav-reverberate --duration=20.25 --impulse-response=rir.wav --additive-signals='noise1.wav,noise2.wav' --snrs='20.0,15.0' "
    "--start-times='0,17.8' input.wav output.wav\n"
    "Options: --impulse-response=<rxfilename> --additive-signals=<rxfilename,...> --snrs=<dB,...> --start-times=<s,...>\n"
    "         --shift-output (true) --normalize-output (true) --duration (0) --volume (0) --input-wave-channel (0)\n"
    "         --rir-channel (0) --noise-channel (0) --config=<file> --verbose --device=<gpu>\n"
    "Not built (refused): --multi-channel-output=true.\n";

std::vector<std::string> SplitCommas(const std::string& s) {
  std::vector<std::string> out;
  if (s.empty()) return out;
  size_t a = 0;
  for (;;) {
    const size_t b = s.find(',', a);
    std::string e = s.substr(a, b == std::string::npos ? std::string::npos : b - a);
    const size_t f = e.find_first_not_of(" \t");
    const size_t l = e.find_last_not_of(" \t");
    if (f != std::string::npos) out.push_back(e.substr(f, l - f + 1));   // empty elements are dropped, as Kaldi's split does
    if (b == std::string::npos) break;
    a = b + 1;
  }
  return out;
}

struct Tool {
  xv_reverb_options o = xv::ReverbDefaults();
  std::string impulse_response, additive_signals, snrs, start_times;
  int verbose = 0, device = -1;
};

// One channel of a wave file, as float; the channel must exist (Kaldi asserts it).
int ReadChannel(const std::string& rx, int channel, const char* what, std::vector<float>* out) {
  xv::Input in;
  in.Open(rx);
  xv::WaveData w;
  xv::ReadWave(in, &w, true);
  const int st = in.Close();
  if (st != 0 && w.samples.empty()) throw xv::KioError("command of " + rx + " exited with status " + std::to_string(st));
  if (st != 0) XWARN("command of " << rx << " exited with status " << st << "; using the " << w.frames() << " samples it wrote");
  if (channel < 0 || channel >= w.channels)
    throw xv::KioError(std::string("the ") + what + " " + rx + " has " + std::to_string(w.channels) + " channels but channel " +
                       std::to_string(channel) + " was asked for");
  const size_t n = w.frames();
  out->resize(n);
  for (size_t i = 0; i < n; ++i) (*out)[i] = (float)w.samples[i * (size_t)w.channels + (size_t)channel];
  return w.rate;
}

int Run(const Tool& t, const std::vector<std::string>& pos) {
  std::vector<float> input;
  const int rate = ReadChannel(pos[0], t.o.input_wave_channel, "input", &input);
  if (input.empty()) throw xv::KioError("the input " + pos[0] + " has no samples");
  std::vector<float> rir;
  if (!t.impulse_response.empty()) {
    const int r = ReadChannel(t.impulse_response, t.o.rir_channel, "impulse response", &rir);
    if (r != rate)
      throw xv::KioError("sampling frequency mismatch: the impulse response " + t.impulse_response + " has " + std::to_string(r) +
                         ", the input " + std::to_string(rate));
    if (rir.empty()) throw xv::KioError("the impulse response " + t.impulse_response + " has no samples");
  }
  const std::vector<std::string> add = SplitCommas(t.additive_signals), snr_s = SplitCommas(t.snrs), start_s = SplitCommas(t.start_times);
  if (add.size() != snr_s.size() || add.size() != start_s.size())
    throw xv::KioError("--additive-signals, --snrs and --start-times must list the same number of elements (" +
                       std::to_string(add.size()) + ", " + std::to_string(snr_s.size()) + ", " + std::to_string(start_s.size()) + ")");
  std::vector<float> noises, snrs, starts;
  std::vector<int64_t> noise_off = {0};
  std::vector<int32_t> add_noise;
  for (size_t i = 0; i < add.size(); ++i) {
    std::vector<float> one;
    const int r = ReadChannel(add[i], t.o.noise_channel, "additive signal", &one);
    if (r != rate)
      throw xv::KioError("sampling frequency mismatch: the additive signal " + add[i] + " has " + std::to_string(r) + ", the input " +
                         std::to_string(rate));
    if (one.empty()) throw xv::KioError("the additive signal " + add[i] + " has no samples");
    noises.insert(noises.end(), one.begin(), one.end());
    noise_off.push_back((int64_t)noises.size());
    add_noise.push_back((int32_t)i);
    snrs.push_back(xv::ToFloat("snrs", snr_s[i]));
    starts.push_back(xv::ToFloat("start-times", start_s[i]));
  }
  xv::ReverbBatch b;
  b.rate = (float)rate;
  b.samples = input.data();
  const int64_t sample_off[2] = {0, (int64_t)input.size()};
  b.sample_off = sample_off;
  b.n_utts = 1;
  const int64_t rir_off[2] = {0, (int64_t)rir.size()};
  const int32_t utt_rir[1] = {0};
  if (!rir.empty()) {
    b.rirs = rir.data();
    b.rir_off = rir_off;
    b.n_rirs = 1;
    b.utt_rir = utt_rir;
  }
  const int32_t utt_add_off[2] = {0, (int32_t)add.size()};
  if (!add.empty()) {
    b.noises = noises.data();
    b.noise_off = noise_off.data();
    b.n_noises = (int)add.size();
    b.utt_add_off = utt_add_off;
    b.add_noise = add_noise.data();
    b.add_snr = snrs.data();
    b.add_start = starts.data();
  }
  const int64_t n_out = std::max<int64_t>(0, xv::ReverbOutputLength(t.o, b.rate, (int64_t)input.size(), (int64_t)rir.size()));
  std::vector<float> out_f((size_t)n_out + 1);
  std::vector<int16_t> out_q((size_t)n_out + 1);
  int64_t out_off[2] = {0, 0}, clipped = 0;
  xv::Reverberate(xv::PickDevice(t.device), t.o, b, out_off, out_f.data(), out_q.data(), &clipped);
  if (clipped > 0) XWARN("clipped " << clipped << " samples out of total " << n_out << "; reduce volume?");
  xv::WriteWaveI16(pos[1], rate, out_q.data(), n_out);
  if (t.verbose >= 1) XLOG("Wrote " << n_out << " samples at " << rate << " Hz to " << pos[1]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Tool t;
  auto flag = [](const char* name, int32_t* to) {   // a boolean kept as the C interface's int32_t
    return xv::Custom(name, [to](const std::string& n, const std::string& v) { return *to = xv::ToBool(n, v), true; });
  };
  xv::CliTool tool = {
      "wav-reverberate", kUsage,
      {xv::String("impulse-response", &t.impulse_response), xv::String("additive-signals", &t.additive_signals), xv::String("snrs", &t.snrs),
       xv::String("start-times", &t.start_times), flag("shift-output", &t.o.shift_output), flag("normalize-output", &t.o.normalize_output),
       xv::Float("duration", &t.o.duration), xv::Float("volume", &t.o.volume), xv::Int("input-wave-channel", &t.o.input_wave_channel),
       xv::Int("rir-channel", &t.o.rir_channel), xv::Int("noise-channel", &t.o.noise_channel),
       xv::Custom("multi-channel-output", [](const std::string& n, const std::string& v) {   // the refusal quotes the value
         if (xv::ToBool(n, v)) throw xv::KioError("--" + n + "=" + v + " is not supported: one output channel is written");
         return true;
       }),
       xv::Int("verbose", &t.verbose), xv::Int("device", &t.device), xv::Bool("print-args", nullptr)},
      2, 2, [&](const std::vector<std::string>& pos) { return Run(t, pos); }};
  tool.underscores = false;
  tool.config_file = true;
  return xv::ToolsMain(argc, argv, {tool}, xv::NameRule::kExact, "wav-reverberate");   // under any name
}
