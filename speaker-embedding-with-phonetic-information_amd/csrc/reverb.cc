#include "reverb.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "device.h"
#include "kio.h"
#include "knobs.h"
#include "reverb_kernels.h"

namespace xv {

xv_reverb_options ReverbDefaults() {
  xv_reverb_options o;
  memset(&o, 0, sizeof o);
  o.shift_output = 1;
  o.normalize_output = 1;
  o.duration = 0.f;
  o.volume = 0.f;
  return o;
}

int64_t ReverbOutputLength(const xv_reverb_options& o, float rate, int64_t n, int64_t rir_len) {
  if (o.duration > 0.f) return (int64_t)((double)rate * (double)o.duration);
  if (o.shift_output || rir_len <= 0) return n;
  return n + rir_len - 1;
}

void Reverberate(int device, const xv_reverb_options& o, const ReverbBatch& b, int64_t* out_off, float* out_f32, int16_t* out_i16,
                 int64_t* clipped, float* device_ms) {
  const int U = b.n_utts;
  if (U < 0 || !b.sample_off || !out_off) throw KioError("wav-reverberate: bad argument");
  if (!(b.rate > 0.f)) throw KioError("wav-reverberate: the sampling rate must be positive");
  if (b.n_rirs < 0 || b.n_noises < 0 || (b.n_rirs > 0 && (!b.rirs || !b.rir_off)) || (b.n_noises > 0 && (!b.noises || !b.noise_off)))
    throw KioError("wav-reverberate: bad argument");
  out_off[0] = 0;
  if (device_ms) *device_ms = 0.f;
  if (U == 0) return;
  if (!b.samples) throw KioError("wav-reverberate: null samples");

  // ---- the plan: one fp32 array of every signal, one RvUtt per utterance
  const int64_t in_total = b.sample_off[U] - b.sample_off[0];
  const int64_t rir_total = b.n_rirs ? b.rir_off[b.n_rirs] - b.rir_off[0] : 0;
  const int64_t noise_total = b.n_noises ? b.noise_off[b.n_noises] - b.noise_off[0] : 0;
  std::vector<float> sig((size_t)(in_total + rir_total + noise_total));
  if (b.is_i16) {
    const int16_t* s = (const int16_t*)b.samples + b.sample_off[0];
    for (int64_t i = 0; i < in_total; ++i) sig[i] = (float)s[i];
  } else {
    memcpy(sig.data(), (const float*)b.samples + b.sample_off[0], (size_t)in_total * 4);
  }
  const int64_t rir_base = in_total, noise_base = in_total + rir_total;
  for (int64_t i = 0; i < rir_total; ++i) sig[rir_base + i] = b.rirs[b.rir_off[0] + i] * (1.0f / 32768.0f);
  if (noise_total) memcpy(sig.data() + noise_base, b.noises + b.noise_off[0], (size_t)noise_total * 4);

  // per RIR: length, peak, early slice; spectra slots are given out below to the ones an FFT utterance uses
  struct Rir {
    int64_t off = 0;
    int len = 0, peak = 0, e0 = 0, e1 = 0, hfull = -1, hearly = -1, P = 0, Pe = 0;
  };
  std::vector<Rir> rirs(b.n_rirs);
  for (int r = 0; r < b.n_rirs; ++r) {
    const int64_t len = b.rir_off[r + 1] - b.rir_off[r];
    if (len < 1) throw KioError("wav-reverberate: empty impulse response");
    if (len > (1 << 24)) throw KioError("wav-reverberate: impulse response too long");
    Rir& R = rirs[r];
    R.off = rir_base + (b.rir_off[r] - b.rir_off[0]);
    R.len = (int)len;
    const float* h = sig.data() + R.off;
    for (int i = 1; i < R.len; ++i)
      if (h[i] > h[R.peak]) R.peak = i;
    R.e0 = std::max(0, R.peak - (int)(0.001 * (double)b.rate));
    R.e1 = std::min(R.len, R.peak + (int)(0.05 * (double)b.rate));
    if (R.e1 <= R.e0) R.e1 = R.e0 + 1;   // rates below 20 Hz
  }

  std::vector<RvUtt> utts(U);
  std::vector<RvAdd> adds;
  std::vector<int64_t> spec_src_off;     // partitions whose spectra rv_rir_spectra computes
  std::vector<int32_t> spec_src_len;
  int64_t y_total = 0, out_total = 0, epart_total = 0, apart_total = 0;
  for (int u = 0; u < U; ++u) {
    RvUtt& T = utts[u];
    memset(&T, 0, sizeof T);
    T.in_off = b.sample_off[u] - b.sample_off[0];
    T.n = b.sample_off[u + 1] - b.sample_off[u];
    if (T.n < 1) throw KioError("wav-reverberate: utterance " + std::to_string(u) + " has no samples");
    const int r = b.utt_rir ? b.utt_rir[u] : -1;
    if (r >= b.n_rirs) throw KioError("wav-reverberate: impulse response index out of range");
    T.ext_len = T.n;
    T.scale = 1.f;
    if (r >= 0) {
      Rir& R = rirs[r];
      T.rir_len = R.len;
      T.h_off = R.off;
      T.e0 = R.e0;
      T.e1 = R.e1;
      T.ext_len = T.n + R.len - 1;
      T.shift = o.shift_output ? R.peak : 0;
      if (R.len > kRvDirectMax && R.hfull < 0) {
        R.hfull = (int)spec_src_off.size();
        R.P = (int)CeilDiv(R.len, kRvH);
        for (int p = 0; p < R.P; ++p) {
          spec_src_off.push_back(R.off + (int64_t)p * kRvH);
          spec_src_len.push_back(std::min(kRvH, R.len - p * kRvH));
        }
        R.hearly = (int)spec_src_off.size();
        R.Pe = (int)CeilDiv(R.e1 - R.e0, kRvH);
        for (int p = 0; p < R.Pe; ++p) {
          spec_src_off.push_back(R.off + R.e0 + (int64_t)p * kRvH);
          spec_src_len.push_back(std::min(kRvH, R.e1 - R.e0 - p * kRvH));
        }
      }
      T.hfull = R.hfull;
      T.P = R.P;
      T.hearly = R.hearly;
      T.Pe = R.Pe;
    }
    if (T.ext_len >= (int64_t)INT32_MAX * kRvH) throw KioError("wav-reverberate: utterance too long");   // int32 block indices
    T.y_off = y_total;
    y_total += T.ext_len;
    T.out_len = ReverbOutputLength(o, b.rate, T.n, T.rir_len);
    if (T.out_len < 0) T.out_len = 0;
    T.out_off = out_total;
    out_total += T.out_len;
    out_off[u + 1] = out_total;
    T.epart_off = epart_total;
    if (T.rir_len > 0) epart_total += T.rir_len > kRvDirectMax ? CeilDiv(T.ext_len, kRvH) : CeilDiv(T.ext_len, kRvDirectChunk);
    T.apart_off = apart_total;
    apart_total += CeilDiv(T.ext_len, kRvChunk);
    T.add_first = (int32_t)adds.size();
    if (b.utt_add_off) {
      if (b.utt_add_off[u + 1] < b.utt_add_off[u]) throw KioError("wav-reverberate: additive-signal offsets must not decrease");
      for (int k = b.utt_add_off[u]; k < b.utt_add_off[u + 1]; ++k) {
        const int ni = b.add_noise[k];
        if (ni < 0 || ni >= b.n_noises) throw KioError("wav-reverberate: additive signal index out of range");
        RvAdd A;
        memset(&A, 0, sizeof A);
        A.off = noise_base + (b.noise_off[ni] - b.noise_off[0]);
        A.len = b.noise_off[ni + 1] - b.noise_off[ni];
        if (A.len < 1) throw KioError("wav-reverberate: empty additive signal");
        A.start = (int64_t)((double)b.add_start[k] * (double)b.rate);
        adds.push_back(A);
      }
    }
    T.add_count = (int32_t)adds.size() - T.add_first;
  }
  if (out_total > 0 && !out_f32) throw KioError("wav-reverberate: null output");

  UseDevice(device, "the reverberation kernels need");
  EventTimer clock(device_ms != nullptr);
  float unasked = 0.f;
  float& kernel_ms = device_ms ? *device_ms : unasked;   // the sum of the kernels' times
  DevBuf d_sig, d_utts, d_adds, d_y;
  d_sig.Upload(sig, "copy signals");
  d_y.Alloc((size_t)y_total * 4);

  // ---- powers of the inputs and of the noises (chunks of kRvChunk samples, added in order)
  std::vector<int64_t> chunk_off;
  std::vector<int32_t> chunk_len;
  std::vector<int64_t> first_chunk;   // per signal: U inputs, then the noises
  auto add_chunks = [&](int64_t off, int64_t len) {
    first_chunk.push_back((int64_t)chunk_off.size());
    for (int64_t c = 0; c < len; c += kRvChunk) {
      chunk_off.push_back(off + c);
      chunk_len.push_back((int32_t)std::min<int64_t>(kRvChunk, len - c));
    }
  };
  for (int u = 0; u < U; ++u) add_chunks(utts[u].in_off, utts[u].n);
  for (int k = 0; k < b.n_noises; ++k) add_chunks(noise_base + (b.noise_off[k] - b.noise_off[0]), b.noise_off[k + 1] - b.noise_off[k]);
  first_chunk.push_back((int64_t)chunk_off.size());
  std::vector<double> power(first_chunk.size() - 1, 0.0);   // mean squares
  {
    DevBuf d_coff, d_clen, d_part;
    d_coff.Upload(chunk_off, "copy chunks");
    d_clen.Upload(chunk_len, "copy chunks");
    d_part.Alloc(chunk_off.size() * 8);
    RvPowerArgs a;
    a.sig = d_sig.as<float>();
    a.chunk_off = d_coff.as<int64_t>();
    a.chunk_len = d_clen.as<int32_t>();
    a.n_chunks = (int)chunk_off.size();
    a.out = d_part.as<double>();
    clock.Start();
    Check(launch_rv_power(a, nullptr), "power kernel launch");
    kernel_ms += clock.Stop();
    std::vector<double> part(chunk_off.size());
    Check(hipMemcpy(part.data(), d_part.p, part.size() * 8, hipMemcpyDeviceToHost), "copy powers");
    for (size_t s = 0; s + 1 < first_chunk.size(); ++s) {
      double sum = 0.0, len = 0.0;
      for (int64_t c = first_chunk[s]; c < first_chunk[s + 1]; ++c) {
        sum += part[c];
        len += chunk_len[c];
      }
      power[s] = len > 0 ? sum / len : 0.0;
    }
  }

  // ---- convolution
  std::vector<double> early(U);
  for (int u = 0; u < U; ++u) early[u] = power[u];
  if (epart_total > 0) {
    DevBuf d_epart, d_tw, d_hspec, d_soff, d_slen;
    d_epart.Alloc((size_t)epart_total * 8);
    std::vector<float> tw(kRvN);
    for (int j = 0; j < kRvN / 2; ++j) {
      tw[2 * j] = (float)cos(2.0 * M_PI * j / kRvN);
      tw[2 * j + 1] = (float)-sin(2.0 * M_PI * j / kRvN);
    }
    d_tw.Upload(tw, "copy twiddles");
    if (!spec_src_off.empty()) {
      d_soff.Upload(spec_src_off, "copy partitions");
      d_slen.Upload(spec_src_len, "copy partitions");
      d_hspec.Alloc(spec_src_off.size() * (size_t)kRvN * sizeof(float2));
      RvRirSpecArgs a;
      a.sig = d_sig.as<float>();
      a.src_off = d_soff.as<int64_t>();
      a.src_len = d_slen.as<int32_t>();
      a.n_items = (int)spec_src_off.size();
      a.twiddle = d_tw.as<float2>();
      a.hspec = d_hspec.as<float2>();
      clock.Start();
      Check(launch_rv_rir_spectra(a, nullptr), "RIR spectra kernel launch");
      kernel_ms += clock.Stop();
    }
    // the block spectra of the signals take 16 bytes per sample: utterances go through in groups of bounded size
    const int64_t kGroupBlocks = std::max(1, DebugKnobInt("reverb_group_blocks", 16384));   // 16384: 512 MiB of spectra
    DevBuf d_xspec;
    int u0 = 0;
    while (u0 < U) {
      WorkItems fft, direct;
      int64_t blocks = 0;
      int u1 = u0;
      for (; u1 < U; ++u1) {
        RvUtt& T = utts[u1];
        if (T.rir_len > kRvDirectMax) {
          const int64_t nb = CeilDiv(T.ext_len, kRvH);
          if (blocks > 0 && blocks + nb > kGroupBlocks) break;
          T.xspec_off = blocks;
          blocks += nb;
          fft.Add(u1, nb);
        } else if (T.rir_len > 0) {
          direct.Add(u1, CeilDiv(T.ext_len, kRvDirectChunk));
        }
      }
      d_utts.Upload(utts, "copy utterances");
      if (blocks > 0) d_xspec.Reserve((size_t)blocks * kRvN * sizeof(float2));
      RvConvArgs a;
      memset(&a, 0, sizeof a);
      a.sig = d_sig.as<float>();
      a.utts = d_utts.as<RvUtt>();
      a.twiddle = d_tw.as<float2>();
      a.hspec = d_hspec.as<float2>();
      a.xspec = d_xspec.as<float2>();
      a.y = d_y.as<float>();
      a.epart = d_epart.as<double>();
      if (fft.size()) {
        fft.Upload();
        a.item_utt = fft.d_unit.as<int32_t>();
        a.item_blk = fft.d_blk.as<int32_t>();
        a.n_items = fft.size();
        clock.Start();
        Check(launch_rv_sig_spectra(a, nullptr), "signal spectra kernel launch");
        Check(launch_rv_conv(a, nullptr), "convolution kernel launch");
        kernel_ms += clock.Stop();
      }
      if (direct.size()) {
        direct.Upload();
        a.item_utt = direct.d_unit.as<int32_t>();
        a.item_blk = direct.d_blk.as<int32_t>();
        a.n_items = direct.size();
        clock.Start();
        Check(launch_rv_conv_direct(a, nullptr), "direct convolution kernel launch");
        kernel_ms += clock.Stop();
      }
      Check(hipDeviceSynchronize(), "convolution kernels");
      u0 = u1;
    }
    std::vector<double> ep((size_t)epart_total);
    Check(hipMemcpy(ep.data(), d_epart.p, ep.size() * 8, hipMemcpyDeviceToHost), "copy early energies");
    for (int u = 0; u < U; ++u) {
      if (utts[u].rir_len <= 0) continue;
      const int64_t c1 = u + 1 < U ? utts[u + 1].epart_off : epart_total;
      double sum = 0.0;
      for (int64_t c = utts[u].epart_off; c < c1; ++c) sum += ep[c];
      early[u] = sum / (double)utts[u].ext_len;
    }
  }

  // ---- scale of each additive signal, mixing, power afterwards
  for (int u = 0; u < U; ++u)
    for (int k = 0; k < utts[u].add_count; ++k) {
      const int gi = utts[u].add_first + k;
      const int ni = b.add_noise[b.utt_add_off[u] + k];
      const double np = power[U + ni];
      const double snr = (double)b.add_snr[b.utt_add_off[u] + k];
      adds[gi].scale = np > 0.0 ? (float)sqrt(pow(10.0, -snr / 10.0) * early[u] / np) : 0.f;
    }
  std::vector<double> after(U, 0.0);
  {
    WorkItems mix;
    for (int u = 0; u < U; ++u) mix.Add(u, CeilDiv(utts[u].ext_len, kRvChunk));
    mix.Upload();
    d_utts.Upload(utts, "copy utterances");
    d_adds.Upload(adds, "copy additive signals");
    DevBuf d_apart;
    d_apart.Alloc((size_t)apart_total * 8);
    RvMixArgs a;
    a.sig = d_sig.as<float>();
    a.utts = d_utts.as<RvUtt>();
    a.adds = d_adds.as<RvAdd>();
    a.item_utt = mix.d_unit.as<int32_t>();
    a.item_blk = mix.d_blk.as<int32_t>();
    a.n_items = mix.size();
    a.y = d_y.as<float>();
    a.apart = d_apart.as<double>();
    clock.Start();
    Check(launch_rv_mix(a, nullptr), "mix kernel launch");
    kernel_ms += clock.Stop();
    std::vector<double> ap((size_t)apart_total);
    Check(hipMemcpy(ap.data(), d_apart.p, ap.size() * 8, hipMemcpyDeviceToHost), "copy powers");
    for (int u = 0; u < U; ++u) {
      const int64_t c1 = u + 1 < U ? utts[u + 1].apart_off : apart_total;
      double sum = 0.0;
      for (int64_t c = utts[u].apart_off; c < c1; ++c) sum += ap[c];
      after[u] = sum / (double)utts[u].ext_len;
    }
  }
  for (int u = 0; u < U; ++u) {
    if (o.volume > 0.f) utts[u].scale = o.volume;
    else if (o.normalize_output) utts[u].scale = after[u] > 0.0 ? (float)sqrt(power[u] / after[u]) : 1.f;
    else utts[u].scale = 1.f;
  }

  // ---- the outputs
  if (out_total == 0) return;
  {
    WorkItems fin;
    for (int u = 0; u < U; ++u) fin.Add(u, CeilDiv(utts[u].out_len, kRvChunk));
    fin.Upload();
    d_utts.Upload(utts, "copy utterances");
    DevBuf d_f32, d_i16, d_clip;
    d_f32.Alloc((size_t)out_total * 4);
    if (out_i16) {
      d_i16.Alloc((size_t)out_total * 2);
      d_clip.Alloc((size_t)U * 8);
      Check(hipMemset(d_clip.p, 0, (size_t)U * 8), "hipMemset");
    }
    RvFinishArgs a;
    a.utts = d_utts.as<RvUtt>();
    a.item_utt = fin.d_unit.as<int32_t>();
    a.item_blk = fin.d_blk.as<int32_t>();
    a.n_items = fin.size();
    a.y = d_y.as<float>();
    a.out_f32 = d_f32.as<float>();
    a.out_i16 = out_i16 ? d_i16.as<int16_t>() : nullptr;
    a.clipped = out_i16 ? d_clip.as<unsigned long long>() : nullptr;
    clock.Start();
    Check(launch_rv_finish(a, nullptr), "finish kernel launch");
    kernel_ms += clock.Stop();
    Check(hipMemcpy(out_f32, d_f32.p, (size_t)out_total * 4, hipMemcpyDeviceToHost), "copy output");
    if (out_i16) {
      Check(hipMemcpy(out_i16, d_i16.p, (size_t)out_total * 2, hipMemcpyDeviceToHost), "copy output");
      if (clipped) {
        std::vector<unsigned long long> c(U);
        Check(hipMemcpy(c.data(), d_clip.p, (size_t)U * 8, hipMemcpyDeviceToHost), "copy clip counts");
        for (int u = 0; u < U; ++u) clipped[u] = (int64_t)c[u];
      }
    } else if (clipped) {
      for (int u = 0; u < U; ++u) clipped[u] = 0;
    }
  }
}

}  // namespace xv
