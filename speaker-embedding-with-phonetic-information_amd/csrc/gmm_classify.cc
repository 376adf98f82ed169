#include "gmm_classify.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "device.h"
#include "gmm_classify_kernels.h"
#include "ubm_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "the UBM kernels need";
// A call's frames go through in parts, as UbmPost's do: a frame's results do not depend on the part it is in.
constexpr int64_t kPart = 1 << 16;

void NeedFull(const char* who, const UbmModel& m) {
  if (!m.full()) throw KioError(std::string(who) + ": the model is a diagonal one; a full-covariance model is needed here");
}

}  // namespace

void UbmFullGselect(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* preselect, int n_in, int n_out,
                    int32_t* idx, float* ll, float* device_ms3) {
  const char* who = "fgmm-gselect";
  if (device_ms3) device_ms3[0] = device_ms3[1] = device_ms3[2] = 0.f;
  NeedFull(who, full);
  const int64_t rows = CheckOffsets(who, row_off, n_utts);
  if (n_out < 1) throw KioError(std::string(who) + ": n must be at least 1");
  if (n_in < 1) throw KioError(std::string(who) + ": the preselection must have at least one Gaussian per frame");
  if (n_in > kUbmMaxSelect)
    throw KioError(std::string(who) + ": the preselection has " + std::to_string(n_in) + " Gaussians per frame, above the device kernels' limit of " +
                   std::to_string(kUbmMaxSelect));
  if (rows == 0) return;
  if (!feats || !preselect || !idx) throw KioError(std::string(who) + ": null buffer");
  CheckUbmSelection(who, full, preselect, rows, n_in);
  UseDevice(full.device(), kWhoNeeds);
  const int n_keep = std::min(n_out, n_in);
  UbmPostDevice dev;
  DevBuf d_idx, d_ll;
  for (int64_t r0 = 0; r0 < rows; r0 += kPart) {
    const int64_t nr = std::min(rows - r0, kPart);
    const size_t kept = (size_t)nr * n_keep;
    d_idx.Reserve(kept * 4);
    if (ll) d_ll.Reserve(kept * 4);
    EventTimer tm(device_ms3 != nullptr, 4);
    UbmFullArgs a;
    dev.Scores(full, feats + (size_t)r0 * full.dim(), preselect + (size_t)r0 * n_in, nr, n_in, &a, &tm);
    UbmRerankArgs r;
    memset(&r, 0, sizeof r);
    r.rows = nr;
    r.n_in = n_in;
    r.n_keep = n_keep;
    r.preselect = a.gselect;
    r.ll = a.ll;
    r.out_idx = d_idx.as<int32_t>();
    r.out_ll = ll ? d_ll.as<float>() : nullptr;
    Check(launch_ubm_full_rerank(r, nullptr), "ubm_full_rerank launch");
    tm.Mark();
    if (device_ms3)
      for (int i = 0; i < 3; ++i) device_ms3[i] += tm.Span(i);
    d_idx.Download(idx + (size_t)r0 * n_keep, kept * 4, "copy the selection");
    if (ll) d_ll.Download(ll + (size_t)r0 * n_keep, kept * 4, "copy the log-likelihoods");
  }
}

void UbmFrameLikes(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* gselect, int n, float* likes,
                   float* device_ms3) {
  const char* who = "get-frame-likes";
  if (device_ms3) device_ms3[0] = device_ms3[1] = device_ms3[2] = 0.f;
  NeedFull(who, full);
  const int64_t rows = CheckOffsets(who, row_off, n_utts);
  if (!gselect) {
    if (full.num_gauss() > kUbmMaxSelect)
      throw KioError(std::string(who) + ": without a Gaussian selection every component is scored, and the model's " + std::to_string(full.num_gauss()) +
                     " are above the device kernels' limit of " + std::to_string(kUbmMaxSelect) + ": pass a selection");
    n = full.num_gauss();
  } else if (n > kUbmMaxSelect) {
    throw KioError(std::string(who) + ": the selection has " + std::to_string(n) + " Gaussians per frame, above the device kernels' limit of " +
                   std::to_string(kUbmMaxSelect));
  }
  CheckUbmSelection(who, full, nullptr, 0, n);
  if (rows == 0) return;
  if (!feats || !likes) throw KioError(std::string(who) + ": null buffer");
  if (gselect) CheckUbmSelection(who, full, gselect, rows, n);
  UseDevice(full.device(), kWhoNeeds);
  std::vector<int32_t> identity;
  if (!gselect) {
    identity.resize((size_t)std::min(rows, kPart) * n);
    for (size_t i = 0; i < identity.size(); ++i) identity[i] = (int32_t)(i % (size_t)n);
  }
  UbmPostDevice dev;
  for (int64_t r0 = 0; r0 < rows; r0 += kPart) {
    const int64_t nr = std::min(rows - r0, kPart);
    dev.Run(full, feats + (size_t)r0 * full.dim(), gselect ? gselect + (size_t)r0 * n : identity.data(), nr, n, 0.f, false, device_ms3);
    dev.logsum.Download(likes + r0, (size_t)nr * 4, "copy the frame likelihoods");
  }
}

void VadFromFrameLikes(int n_classes, const float* const* likes, int64_t rows, const float* priors, const int32_t* map, float* out) {
  if (n_classes < 1 || rows < 0 || !likes || (rows > 0 && !out)) throw KioError("compute-vad-from-frame-likes: bad argument");
  std::vector<float> log_prior((size_t)n_classes, 0.f);
  for (int j = 0; j < n_classes; ++j) {
    if (!likes[j] && rows > 0) throw KioError("compute-vad-from-frame-likes: null buffer");
    if (!priors) continue;
    if (!(priors[j] > 0.f)) throw KioError("compute-vad-from-frame-likes: prior " + std::to_string(j) + " is not positive");
    log_prior[j] = logf(priors[j]);
  }
  for (int64_t t = 0; t < rows; ++t) {
    int best = 0;
    float best_score = likes[0][t] + log_prior[0];
    for (int j = 1; j < n_classes; ++j) {
      const float s = likes[j][t] + log_prior[j];
      if (s > best_score) {
        best_score = s;
        best = j;
      }
    }
    out[t] = (float)(map ? map[best] : best);
  }
}

void MergeVads(const float* a, const float* b, int64_t rows, const int32_t* map_triples, int n_triples, float* out) {
  if (rows < 0 || n_triples < 0 || (rows > 0 && (!a || !b || !out)) || (n_triples > 0 && !map_triples)) throw KioError("merge-vads: bad argument");
  if (n_triples == 0) {
    for (int64_t t = 0; t < rows; ++t) out[t] = (a[t] == 1.f && b[t] == 1.f) ? 1.f : 0.f;
    return;
  }
  std::map<std::pair<int32_t, int32_t>, int32_t> m;
  for (int i = 0; i < n_triples; ++i) m[std::make_pair(map_triples[3 * i], map_triples[3 * i + 1])] = map_triples[3 * i + 2];
  for (int64_t t = 0; t < rows; ++t) {
    const auto it = m.find(std::make_pair((int32_t)a[t], (int32_t)b[t]));
    if (it == m.end())
      throw KioError("merge-vads: the map has no entry for the pair (" + std::to_string((int32_t)a[t]) + ", " + std::to_string((int32_t)b[t]) + ")");
    out[t] = (float)it->second;
  }
}

}  // namespace xv
