// compute-mfcc-feats / compute-vad - drop-in command lines for stage 1 of the recipes (egs/sre/v2/run_sre10.sh:78-90 through
// steps/make_mfcc.sh:126-129 and sid/compute_vad_decision.sh:56-57); one executable, dispatching on its name:
//   compute-mfcc-feats [options] <wav-rspecifier> <feats-wspecifier>
//   compute-vad [options] <feats-rspecifier> <vad-wspecifier>
// The arithmetic runs on the HIP device through libxvec_hip.so (feat.h); without a GPU the tools fail (exit 255).  Option
// names, defaults, log lines and exit codes follow Kaldi's tools (0 iff something was written); options that would change
// the numbers and are not built are refused.  One GPU context per process; batches are sized by sample count.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat.h"
#include "fuse_wav.h"
#include "kio.h"
#include "knobs.h"
#include "wave.h"

namespace {

const char* Usage(bool vad) {
  if (vad)
    return "This program reads input features and writes out, for each utterance,\n"
           "a vector of floats that are 1.0 if we judge the frame voiced and 0.0\n"
           "otherwise (energy-based, column 0 of the features is the log energy).\n"
           "Usage: compute-vad [options] <feats-rspecifier> <vad-wspecifier>\n"
           "Options: --vad-energy-threshold (5.0) --vad-energy-mean-scale (0.5) --vad-frames-context (0)\n"
           "         --vad-proportion-threshold (0.6) --config=<file> --device=<gpu>\n";
  return "Create MFCC feature files.\n"
         "Usage: compute-mfcc-feats [options...] <wav-rspecifier> <feats-wspecifier>\n"
         "Options: --sample-frequency --frame-length --frame-shift --dither --preemphasis-coefficient --remove-dc-offset\n"
         "         --window-type --blackman-coeff --round-to-power-of-two --snip-edges --num-mel-bins --low-freq --high-freq\n"
         "         --num-ceps --cepstral-lifter --use-energy --raw-energy --energy-floor --channel --min-duration\n"
         "         --subtract-mean --output-format=kaldi --config=<file> --verbose --device=<gpu>\n"
         "Not built (refused): --vtln-map, --vtln-warp != 1, --htk-compat=true, --output-format=htk, resampling.\n";
}

constexpr int64_t kBatchSamples = 16 << 20;   // samples per device call (32 MiB of 16-bit PCM)
constexpr int64_t kBatchFloats = 16 << 20;    // feature values per device call of compute-vad

int ComputeMfcc(const xv::MfccToolOptions& t, const std::vector<std::string>& pos) {
  const int device = xv::PickDevice(t.device);
  xv::MfccComputer mc(device, t.mfcc);
  xv::SequentialWaveReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_utts = 0, num_success = 0, num_fused = 0;
  std::vector<std::string> keys;
  std::vector<std::vector<int16_t>> waves;               // per utterance; empty while its job waits for the device
  std::vector<std::unique_ptr<xv::WavJob>> jobs;         // per utterance; null for a plain entry
  int64_t pending = 0;
  std::vector<int16_t> samples;
  std::vector<int64_t> off = {0};
  std::vector<uint64_t> seeds;
  std::vector<float> feats;
  std::vector<int32_t> row_off;
  // wav-reverberate lines (fuse_wav.h): read here, reverberated on the device with the batch
  const bool fuse = xv::DebugKnobInt("fuse_wav", 1) != 0;
  std::unique_ptr<xv::WavJob> taken;
  if (fuse)
    reader.SetEntryHook([&](const std::string& rx, xv::WaveData* w, std::string* error) {
      xv::FusedWav p;
      if (!xv::RecognizeWavPipeline(rx, &p)) return false;
      taken.reset(new xv::WavJob);
      try {
        xv::LoadWavJob(p, taken.get());
        w->rate = taken->rate;
        w->channels = 1;
        w->samples.clear();
      } catch (const xv::KioError& e) {
        *error = e.what();
        taken.reset();
      }
      return true;
    });
  auto flush = [&] {
    if (keys.empty()) return;
    std::vector<xv::WavJob*> run;
    for (auto& j : jobs)
      if (j) run.push_back(j.get());
    xv::RunWavJobs(device, run);
    for (size_t u = 0; u < keys.size(); ++u) {
      if (jobs[u]) {
        if (jobs[u]->clipped > 0) XWARN("clipped " << jobs[u]->clipped << " samples out of total " << jobs[u]->out.size() << " of utterance " << keys[u]);
        waves[u].swap(jobs[u]->out);
        jobs[u].reset();
      }
      samples.insert(samples.end(), waves[u].begin(), waves[u].end());
      off.push_back((int64_t)samples.size());
    }
    row_off.assign(keys.size() + 1, 0);
    mc.Compute(samples.data(), true, off.data(), (int)keys.size(), seeds.data(), &feats, row_off.data());
    const int nc = t.mfcc.num_ceps;
    for (size_t u = 0; u < keys.size(); ++u) {
      xv::Matrix m;
      m.rows = row_off[u + 1] - row_off[u];
      m.cols = m.rows ? nc : 0;
      m.data.assign(feats.begin() + (size_t)row_off[u] * nc, feats.begin() + (size_t)row_off[u + 1] * nc);
      if (t.subtract_mean && m.rows > 0) {
        for (int c = 0; c < nc; ++c) {
          double s = 0;
          for (int r = 0; r < m.rows; ++r) s += m.data[(size_t)r * nc + c];
          const float mean = (float)(s / m.rows);
          for (int r = 0; r < m.rows; ++r) m.data[(size_t)r * nc + c] -= mean;
        }
      }
      if (m.rows == 0) XWARN("No frames fit in the " << (off[u + 1] - off[u]) << " samples of utterance " << keys[u] << "; writing an empty matrix");
      writer.WriteMat(keys[u], m);
      if (t.verbose >= 2) XLOG("Processed features for key " << keys[u]);
      ++num_success;
    }
    keys.clear();
    waves.clear();
    jobs.clear();
    pending = 0;
    samples.clear();
    off.assign(1, 0);
    seeds.clear();
  };
  std::string key, err, warn;
  xv::WaveData w;
  std::vector<int16_t> one;
  for (;;) {
    taken.reset();
    if (!reader.Next(&key, &w, &err)) break;
    ++num_utts;
    if (!err.empty()) {
      if (!reader.permissive()) throw xv::KioError("Failed to read wave data for key " + key + ": " + err);
      XWARN("Skipping utterance " << key << ": " << err);
      continue;
    }
    const double duration = w.rate > 0 ? (double)(taken ? (size_t)taken->out_len : w.frames()) / w.rate : 0.0;
    if (duration < t.min_duration) {
      XWARN("File: " << key << " is too short (" << duration << " sec): producing no output.");
      continue;
    }
    if ((float)w.rate != t.mfcc.sample_frequency) {
      XWARN("Sample frequency mismatch for utterance " << key << ": the file has " << w.rate << ", --sample-frequency is "
            << t.mfcc.sample_frequency << " (there is no resampling); skipping it");
      continue;
    }
    warn.clear();
    try {
      xv::SelectChannel(w, t.channel, &one, &warn);
    } catch (const xv::KioError& e) {
      XWARN("Utterance " << key << ": " << e.what());
      continue;
    }
    if (!warn.empty()) XWARN(warn << " (utterance " << key << ")");
    keys.push_back(key);
    pending += taken ? taken->out_len : (int64_t)one.size();
    if (taken) {
      ++num_fused;
      waves.emplace_back();
    } else {
      waves.push_back(one);
    }
    jobs.push_back(std::move(taken));
    seeds.push_back(xv::UttSeed(key.c_str()));
    if (pending >= kBatchSamples) flush();
  }
  flush();
  writer.Close();
  XLOG("Took over " << num_fused << " wav-reverberate entries of the wave table" << (fuse ? "" : " (fuse_wav=0)"));
  XLOG(" Done " << num_success << " out of " << num_utts << " utterances.");
  return num_success != 0 ? 0 : 1;
}

int ComputeVad(const xv_vad_options& o, int device, const std::vector<std::string>& pos) {
  const int dev = xv::PickDevice(device);
  xv::SequentialMatrixReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_done = 0, num_err = 0, num_unvoiced = 0;
  double tot_length = 0, tot_decision = 0;
  std::vector<std::string> keys;
  std::vector<float> feats, dec;
  std::vector<int32_t> off = {0};
  int dim = 0;
  auto flush = [&] {
    if (keys.empty()) return;
    dec.assign((size_t)off.back(), 0.f);
    xv::VadEnergy(dev, o, feats.data(), off.data(), (int)keys.size(), dim, dec.data());
    for (size_t u = 0; u < keys.size(); ++u) {
      const float* v = dec.data() + off[u];
      const int n = off[u + 1] - off[u];
      double sum = 0;
      for (int i = 0; i < n; ++i) sum += v[i];
      if (sum == 0.0) {
        XWARN("No frames were judged voiced for utterance " << keys[u]);
        ++num_unvoiced;
      } else {
        ++num_done;
      }
      tot_decision += sum;
      tot_length += n;
      writer.WriteVec(keys[u], v, n);
    }
    keys.clear();
    feats.clear();
    off.assign(1, 0);
  };
  std::string key, err;
  xv::Matrix m;
  while (reader.Next(&key, &m, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read features for key " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (m.rows == 0) {
      XWARN("Empty features for utterance " << key);
      ++num_err;
      continue;
    }
    if (dim != 0 && m.cols != dim) flush();   // a table may mix dimensions; a batch may not
    dim = m.cols;
    keys.push_back(key);
    feats.insert(feats.end(), m.Data(), m.Data() + (size_t)m.rows * m.cols);
    off.push_back(off.back() + m.rows);
    if ((int64_t)feats.size() >= kBatchFloats) flush();
  }
  flush();
  writer.Close();
  XLOG("Applied energy based voice activity detection; Done " << (num_done + num_unvoiced) << " utterances, " << num_err
       << " had empty features, and " << num_unvoiced << " were completely unvoiced.");
  XLOG("Proportion of voiced frames was " << (tot_length > 0 ? tot_decision / tot_length : 0.0) << " over " << tot_length << " frames.");
  return num_done + num_unvoiced != 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  xv::MfccToolOptions t;
  t.mfcc = xv::MfccDefaults();
  xv_vad_options vo = xv::VadDefaults();
  int vad_device = -1;
  // the options themselves are the library's (feat.h), refusals included
  std::vector<xv::CliTool> tools = {
      {"compute-vad", Usage(true),
       {xv::Custom("", [&](const std::string& n, const std::string& v) { return xv::SetVadOption(n, v, &vo); }), xv::LaxInt("device", &vad_device),
        xv::Ignored("verbose"), xv::Ignored("print-args")},
       2, 2, [&](const Pos& pos) { return ComputeVad(vo, vad_device, pos); }, "vad"},
      {"compute-mfcc-feats", Usage(false), {xv::Custom("", [&](const std::string& n, const std::string& v) { return xv::SetMfccOption(n, v, &t); })},
       0, -1, [&](const Pos& pos) {
         (void)xv::BuildMfccTables(t.mfcc);   // option errors before the argument count and before any device is touched
         return pos.size() != 2 ? xv::kUsageError : ComputeMfcc(t, pos);
       }},
  };
  for (xv::CliTool& tool : tools) {
    tool.underscores = false;
    tool.config_file = true;
  }
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kContains, "compute-mfcc-feats");
}
