#include "feat.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <limits>

#include "cli.h"
#include "device.h"
#include "feat_kernels.h"
#include "kio.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "the feature kernels need";

double MelScale(double f) { return 1127.0 * log(1.0 + f / 700.0); }

}  // namespace

xv_mfcc_options MfccDefaults() {
  xv_mfcc_options o;
  memset(&o, 0, sizeof o);
  o.sample_frequency = 16000.f;
  o.frame_length_ms = 25.f;
  o.frame_shift_ms = 10.f;
  o.dither = 1.f;
  o.preemphasis_coefficient = 0.97f;
  o.blackman_coeff = 0.42f;
  o.remove_dc_offset = 1;
  o.window_type = 0;
  o.round_to_power_of_two = 1;
  o.snip_edges = 1;
  o.num_mel_bins = 23;
  o.low_freq = 20.f;
  o.high_freq = 0.f;
  o.num_ceps = 13;
  o.cepstral_lifter = 22.f;
  o.use_energy = 1;
  o.raw_energy = 1;
  o.energy_floor = 0.f;
  return o;
}

xv_vad_options VadDefaults() {
  xv_vad_options o;
  o.vad_energy_threshold = 5.f;
  o.vad_energy_mean_scale = 0.5f;
  o.vad_proportion_threshold = 0.6f;
  o.vad_frames_context = 0;
  return o;
}

MfccGeometry MfccGeometryOf(const xv_mfcc_options& o) {
  MfccGeometry g;
  if (!(o.sample_frequency > 0.f)) throw KioError("MFCC options: sample-frequency must be positive");
  // Kaldi: static_cast<int32>(samp_freq * 0.001 * frame_length_ms)
  g.frame_len = (int)((double)o.sample_frequency * 0.001 * (double)o.frame_length_ms);
  g.frame_shift = (int)((double)o.sample_frequency * 0.001 * (double)o.frame_shift_ms);
  if (g.frame_len < 2 || g.frame_shift < 1) throw KioError("MFCC options: frame-length / frame-shift give no usable window");
  if (!o.round_to_power_of_two) throw KioError("--round-to-power-of-two=false is not supported (the FFT is a power-of-two one)");
  g.padded = 1;
  while (g.padded < g.frame_len) { g.padded <<= 1; ++g.log2_padded; }
  if (g.padded > kMfccMaxPadded)
    throw KioError("MFCC options: a window of " + std::to_string(g.frame_len) + " samples is larger than the kernel's FFT (" +
                   std::to_string(kMfccMaxPadded) + ")");
  if (o.window_type < 0 || o.window_type > 4) throw KioError("MFCC options: unknown window type");
  if (o.num_mel_bins < 3) throw KioError("MFCC options: num-mel-bins must be at least 3");
  if (o.num_ceps < 1 || o.num_ceps > o.num_mel_bins)
    throw KioError("MFCC options: num-ceps must be in [1, num-mel-bins] (" + std::to_string(o.num_ceps) + " vs " +
                   std::to_string(o.num_mel_bins) + ")");
  if (o.preemphasis_coefficient < 0.f || o.preemphasis_coefficient > 1.f) throw KioError("MFCC options: preemphasis-coefficient must be in [0, 1]");
  if (o.energy_floor < 0.f) throw KioError("MFCC options: energy-floor must not be negative");
  return g;
}

int64_t MfccNumFrames(const xv_mfcc_options& o, int64_t n) {
  const MfccGeometry g = MfccGeometryOf(o);
  if (n < 0) n = 0;
  if (o.snip_edges) return n < g.frame_len ? 0 : 1 + (n - g.frame_len) / g.frame_shift;
  return (n + g.frame_shift / 2) / g.frame_shift;
}

MfccTables BuildMfccTables(const xv_mfcc_options& o) {
  MfccTables t;
  t.g = MfccGeometryOf(o);
  const int L = t.g.frame_len, P = t.g.padded;
  // tables are evaluated in double and rounded once
  t.window.resize(L);
  const double a = 2.0 * M_PI / (L - 1);
  for (int i = 0; i < L; ++i) {
    double w;
    switch (o.window_type) {
      case 0: w = pow(0.5 - 0.5 * cos(a * i), 0.85); break;
      case 1: w = 0.54 - 0.46 * cos(a * i); break;
      case 2: w = 0.5 - 0.5 * cos(a * i); break;
      case 3: w = 1.0; break;
      default: w = (double)o.blackman_coeff - 0.5 * cos(a * i) + (0.5 - (double)o.blackman_coeff) * cos(2 * a * i); break;
    }
    t.window[i] = (float)w;
  }
  t.twiddle.resize(P);
  for (int j = 0; j < P / 2; ++j) {
    t.twiddle[2 * j] = (float)cos(2.0 * M_PI * j / P);
    t.twiddle[2 * j + 1] = (float)-sin(2.0 * M_PI * j / P);
  }
  // mel bank (Kaldi's MelBanks without VTLN): triangles on the mel axis over FFT bins 0 .. P/2 - 1
  const double nyquist = 0.5 * (double)o.sample_frequency;
  const double low = o.low_freq;
  const double high = o.high_freq > 0.f ? (double)o.high_freq : nyquist + (double)o.high_freq;
  if (low < 0.0 || low >= nyquist || high <= 0.0 || high > nyquist || high <= low)
    throw KioError("Bad values in options: low-freq " + std::to_string(low) + " and high-freq " + std::to_string(high) +
                   " vs. nyquist " + std::to_string(nyquist));
  const int nb = o.num_mel_bins, nfft = P / 2;
  const double bin_width = (double)o.sample_frequency / P;
  const double mel_low = MelScale(low), mel_high = MelScale(high);
  const double delta = (mel_high - mel_low) / (nb + 1);
  t.mel_first.assign(nb, 0);
  t.mel_len.assign(nb, 0);
  t.mel_woff.assign(nb, 0);
  for (int b = 0; b < nb; ++b) {
    const double left = mel_low + b * delta, center = left + delta, right = center + delta;
    int first = -1, last = -1;
    std::vector<float> w;
    for (int i = 0; i < nfft; ++i) {
      const double mel = MelScale(bin_width * i);
      if (mel > left && mel < right) {
        const double v = mel <= center ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first < 0) first = i;
        last = i;
        w.push_back((float)v);
      }
    }
    // Kaldi asserts here; an empty bin would read log(FLT_EPSILON) for ever.  Bins b and b + 2 do not overlap, so with no
    // empty bin num-mel-bins is at most 2 * P/2 = P: the kernel keeps the log mel energies in an LDS plane of P floats.
    if (first < 0)
      throw KioError("MFCC options: mel bin " + std::to_string(b) + " of " + std::to_string(nb) + " contains no FFT bin (" +
                     std::to_string(nfft) + " bins of " + std::to_string(bin_width) + " Hz): You may have set --num-mel-bins too large.");
    t.mel_woff[b] = (int32_t)t.mel_w.size();
    t.mel_first[b] = first;
    t.mel_len[b] = last - first + 1;
    t.mel_w.insert(t.mel_w.end(), w.begin(), w.end());
  }
  // DCT-II, orthonormal (Kaldi's ComputeDctMatrix), first num_ceps rows, stored transposed
  const int nc = o.num_ceps;
  t.dct_t.resize((size_t)nb * nc);
  for (int k = 0; k < nc; ++k)
    for (int n = 0; n < nb; ++n) {
      const double v = k == 0 ? sqrt(1.0 / nb) : sqrt(2.0 / nb) * cos(M_PI / nb * (n + 0.5) * k);
      t.dct_t[(size_t)n * nc + k] = (float)v;
    }
  t.lifter.resize(nc);
  for (int i = 0; i < nc; ++i)
    t.lifter[i] = o.cepstral_lifter != 0.f ? (float)(1.0 + 0.5 * (double)o.cepstral_lifter * sin(M_PI * i / (double)o.cepstral_lifter)) : 1.f;
  return t;
}

uint64_t UttSeed(const char* key) {
  uint64_t h = 0xcbf29ce484222325ULL;
  for (const unsigned char* p = (const unsigned char*)key; p && *p; ++p) {
    h ^= *p;
    h *= 0x100000001b3ULL;
  }
  return h;
}

struct MfccComputer::Impl {
  int device = 0;
  MfccTables t;
  DevBuf window, twiddle, mel_w, dct_t, lifter, mel_first, mel_len, mel_woff;
  // of one batch: they grow with a quarter to spare, so that batches of slowly rising size do not reallocate every time
  static constexpr DevBuf::Growth kSpare = DevBuf::Growth::kQuarterMore;
  DevBuf samples{kSpare}, sample_off{kSpare}, row_off{kSpare}, seeds{kSpare}, out{kSpare};
};

MfccComputer::MfccComputer(int device, const xv_mfcc_options& o) : p_(nullptr), o_(o) {
  MfccTables t = BuildMfccTables(o);   // option errors come before any device is touched
  UseDevice(device, kWhoNeeds);
  p_ = new Impl;
  p_->device = device;
  p_->t = std::move(t);
  try {
    const MfccTables& tt = p_->t;
    p_->window.Upload(tt.window, "copy window");
    p_->twiddle.Upload(tt.twiddle, "copy twiddles");
    p_->mel_w.Upload(tt.mel_w, "copy mel weights");
    p_->dct_t.Upload(tt.dct_t, "copy DCT");
    p_->lifter.Upload(tt.lifter, "copy lifter");
    p_->mel_first.Upload(tt.mel_first, "copy mel bank");
    p_->mel_len.Upload(tt.mel_len, "copy mel bank");
    p_->mel_woff.Upload(tt.mel_woff, "copy mel bank");
  } catch (...) {
    delete p_;
    throw;
  }
}

MfccComputer::~MfccComputer() { delete p_; }

void MfccComputer::Compute(const void* samples, bool is_i16, const int64_t* sample_off, int n_utts, const uint64_t* seeds,
                           std::vector<float>* out, int32_t* row_off, float* device_ms) {
  if (n_utts < 0 || !sample_off || !row_off || !out) throw EngineError("MfccComputer: bad argument");
  if (o_.dither != 0.f && !seeds && n_utts > 0) throw EngineError("MFCC with dither needs a seed per utterance");
  const MfccGeometry& g = p_->t.g;
  int64_t rows = 0;
  row_off[0] = 0;
  for (int u = 0; u < n_utts; ++u) {
    const int64_t n = sample_off[u + 1] - sample_off[u];
    if (n < 0) throw EngineError("MfccComputer: sample offsets must not decrease");
    rows += o_.snip_edges ? (n < g.frame_len ? 0 : 1 + (n - g.frame_len) / g.frame_shift) : (n + g.frame_shift / 2) / g.frame_shift;
    if (rows > std::numeric_limits<int32_t>::max() / 64) throw EngineError("MfccComputer: batch too large; split it");
    row_off[u + 1] = (int32_t)rows;
  }
  out->assign((size_t)rows * o_.num_ceps, 0.f);
  if (device_ms) *device_ms = 0.f;
  if (rows == 0) return;
  Check(hipSetDevice(p_->device), "hipSetDevice");
  const int64_t total = sample_off[n_utts] - sample_off[0];
  const size_t esz = is_i16 ? 2 : 4;
  // offsets relative to the first sample of the batch
  std::vector<int64_t> rel(n_utts + 1);
  for (int u = 0; u <= n_utts; ++u) rel[u] = sample_off[u] - sample_off[0];
  p_->samples.Upload((const char*)samples + (size_t)sample_off[0] * esz, (size_t)total * esz, "copy samples");
  p_->sample_off.Upload(rel, "copy sample offsets");
  p_->row_off.Upload(row_off, (size_t)(n_utts + 1) * 4, "copy row offsets");
  if (o_.dither != 0.f) p_->seeds.Upload(seeds, (size_t)n_utts * 8, "copy seeds");
  p_->out.Reserve((size_t)rows * o_.num_ceps * 4);
  MfccArgs a;
  memset(&a, 0, sizeof a);
  a.samples = p_->samples.p;
  a.sample_off = p_->sample_off.as<int64_t>();
  a.row_off = p_->row_off.as<int32_t>();
  a.utt_seed = p_->seeds.as<uint64_t>();
  a.n_utts = n_utts;
  a.total_frames = (int)rows;
  a.frame_len = g.frame_len;
  a.frame_shift = g.frame_shift;
  a.padded = g.padded;
  a.log2_padded = g.log2_padded;
  a.snip_edges = o_.snip_edges ? 1 : 0;
  a.dither = o_.dither;
  a.preemph = o_.preemphasis_coefficient;
  a.remove_dc = o_.remove_dc_offset ? 1 : 0;
  a.raw_energy = o_.raw_energy ? 1 : 0;
  a.use_energy = o_.use_energy ? 1 : 0;
  a.has_energy_floor = o_.energy_floor > 0.f ? 1 : 0;
  a.log_energy_floor = o_.energy_floor > 0.f ? logf(o_.energy_floor) : 0.f;
  a.window = p_->window.as<float>();
  a.twiddle = p_->twiddle.as<float>();
  a.num_bins = o_.num_mel_bins;
  a.num_ceps = o_.num_ceps;
  a.mel_first = p_->mel_first.as<int32_t>();
  a.mel_len = p_->mel_len.as<int32_t>();
  a.mel_woff = p_->mel_woff.as<int32_t>();
  a.mel_w = p_->mel_w.as<float>();
  a.dct_t = p_->dct_t.as<float>();
  a.lifter = p_->lifter.as<float>();
  a.out = p_->out.as<float>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(is_i16 ? launch_mfcc_i16(a, nullptr) : launch_mfcc_f32(a, nullptr), "MFCC kernel launch");
  if (device_ms) *device_ms = tm.Stop();
  p_->out.Download(out->data(), out->size() * 4, "copy features");
}

void VadEnergy(int device, const xv_vad_options& o, const float* feats, const int32_t* row_off, int n_utts, int dim, float* out) {
  if (n_utts < 0 || dim < 1 || !row_off) throw EngineError("VadEnergy: bad argument");
  if (o.vad_frames_context < 0) throw KioError("--vad-frames-context must not be negative");
  if (!(o.vad_proportion_threshold > 0.f && o.vad_proportion_threshold < 1.f))
    throw KioError("--vad-proportion-threshold must be in (0, 1)");
  for (int u = 0; u < n_utts; ++u)
    if (row_off[u + 1] < row_off[u]) throw EngineError("VadEnergy: row offsets must not decrease");
  if (n_utts > 0 && row_off[0] != 0) throw EngineError("VadEnergy: row offsets must start at 0");
  UseDevice(device, kWhoNeeds);
  const int rows = n_utts > 0 ? row_off[n_utts] : 0;
  if (rows == 0) return;
  DevBuf df, doff, dthr, dout;
  df.Upload(feats, (size_t)rows * dim * 4, "copy features");
  doff.Upload(row_off, (size_t)(n_utts + 1) * 4, "copy row offsets");
  dthr.Reserve((size_t)n_utts * 4);
  dout.Reserve((size_t)rows * 4);
  VadArgs a;
  a.feats = df.as<float>();
  a.row_off = doff.as<int32_t>();
  a.n_utts = n_utts;
  a.total_rows = rows;
  a.dim = dim;
  a.energy_threshold = o.vad_energy_threshold;
  a.energy_mean_scale = o.vad_energy_mean_scale;
  a.proportion_threshold = o.vad_proportion_threshold;
  a.frames_context = o.vad_frames_context;
  a.thr = dthr.as<float>();
  a.out = dout.as<float>();
  Check(launch_vad_energy(a, nullptr), "VAD kernel launch");
  dout.Download(out, (size_t)rows * 4, "copy VAD decisions");
}

// ---------------------------------------------------------------------------------------------- options
namespace {

[[noreturn]] void Refuse(const std::string& name, const std::string& v, const char* why) {
  throw KioError("--" + name + "=" + v + " is not supported: " + why);
}

}  // namespace

bool SetMfccOption(const std::string& n, const std::string& v, MfccToolOptions* t) {
  xv_mfcc_options& o = t->mfcc;
  if (n == "sample-frequency") o.sample_frequency = ToFloat(n, v);
  else if (n == "frame-length") o.frame_length_ms = ToFloat(n, v);
  else if (n == "frame-shift") o.frame_shift_ms = ToFloat(n, v);
  else if (n == "dither") o.dither = ToFloat(n, v);
  else if (n == "preemphasis-coefficient") o.preemphasis_coefficient = ToFloat(n, v);
  else if (n == "remove-dc-offset") o.remove_dc_offset = ToBool(n, v);
  else if (n == "window-type") {
    static const char* names[] = {"povey", "hamming", "hanning", "rectangular", "blackman"};
    int k = -1;
    for (int i = 0; i < 5; ++i)
      if (v == names[i]) k = i;
    if (k < 0) throw KioError("Invalid window type " + v);
    o.window_type = k;
  } else if (n == "blackman-coeff") o.blackman_coeff = ToFloat(n, v);
  else if (n == "round-to-power-of-two") {
    o.round_to_power_of_two = ToBool(n, v);
    if (!o.round_to_power_of_two) Refuse(n, v, "the FFT on the device is a power-of-two one");
  } else if (n == "snip-edges") o.snip_edges = ToBool(n, v);
  else if (n == "num-mel-bins") o.num_mel_bins = ToInt(n, v);
  else if (n == "low-freq") o.low_freq = ToFloat(n, v);
  else if (n == "high-freq") o.high_freq = ToFloat(n, v);
  else if (n == "num-ceps") o.num_ceps = ToInt(n, v);
  else if (n == "cepstral-lifter") o.cepstral_lifter = ToFloat(n, v);
  else if (n == "use-energy") o.use_energy = ToBool(n, v);
  else if (n == "raw-energy") o.raw_energy = ToBool(n, v);
  else if (n == "energy-floor") o.energy_floor = ToFloat(n, v);
  else if (n == "channel") t->channel = ToInt(n, v);
  else if (n == "min-duration") t->min_duration = ToFloat(n, v);
  else if (n == "subtract-mean") t->subtract_mean = ToBool(n, v);
  else if (n == "verbose") t->verbose = ToInt(n, v);
  else if (n == "device") t->device = ToInt(n, v);
  else if (n == "print-args") (void)ToBool(n, v);
  else if (n == "output-format") {
    if (v != "kaldi") Refuse(n, v, "only Kaldi tables are written");
  } else if (n == "vtln-map" || n == "utt2spk") Refuse(n, v, "VTLN is not built");
  else if (n == "vtln-warp") {
    if (ToFloat(n, v) != 1.f) Refuse(n, v, "VTLN is not built");
  } else if (n == "vtln-low" || n == "vtln-high") (void)ToFloat(n, v);   // only read with a warp factor
  else if (n == "htk-compat") {
    if (ToBool(n, v)) Refuse(n, v, "HTK-compatible features are not built");
  } else if (n == "allow-downsample" || n == "allow-upsample") {
    if (ToBool(n, v)) Refuse(n, v, "there is no resampling; the file's rate must equal --sample-frequency");
  } else if (n == "debug-mel") (void)ToBool(n, v);
  else return false;
  return true;
}

bool SetVadOption(const std::string& n, const std::string& v, xv_vad_options* o) {
  if (n == "vad-energy-threshold") o->vad_energy_threshold = ToFloat(n, v);
  else if (n == "vad-energy-mean-scale") o->vad_energy_mean_scale = ToFloat(n, v);
  else if (n == "vad-proportion-threshold") o->vad_proportion_threshold = ToFloat(n, v);
  else if (n == "vad-frames-context") o->vad_frames_context = ToInt(n, v);
  else return false;
  return true;
}

}  // namespace xv
