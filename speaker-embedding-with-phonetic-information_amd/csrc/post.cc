#include "post.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "device.h"
#include "plda.h"
#include "post_kernels.h"
#include "ubm.h"
#include "ubm_train_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "logprob-to-post needs";

size_t Tri(int d) { return (size_t)d * (d + 1) / 2; }

}  // namespace

int64_t LogprobPostDefaultBudget(int cols) {
  const int64_t rows = (int64_t)(kPostLaunchBytes / ((size_t)(cols < 1 ? 1 : cols) * 4));
  return rows < 1 ? 1 : rows;
}

void LogprobToPost(int device, const float* logprobs, const int32_t* row_off, int n_utts, int cols, const uint64_t* utt_seed, float min_post,
                   bool random_prune, int64_t frame_budget, bool timed, LogprobPostResult* out) {
  *out = LogprobPostResult();
  if (cols < 1) throw KioError("logprob-to-post: bad argument");
  if (min_post != min_post) throw KioError("logprob-to-post: --min-post is not a number");
  const int64_t rows = CheckOffsets("logprob-to-post", row_off, n_utts);
  out->off.assign((size_t)rows + 1, 0);
  if (rows == 0) return;
  const bool draws = random_prune && min_post > 0.f;
  if (!logprobs || (draws && !utt_seed)) throw KioError("logprob-to-post: null input");
  UseDevice(device, kWhoNeeds);
  int64_t budget = frame_budget > 0 ? frame_budget : LogprobPostDefaultBudget(cols);
  budget = std::min(budget, std::max<int64_t>(1, (int64_t)INT32_MAX / cols));   // the pairs of a launch fit an int32
  budget = std::min(budget, rows);
  DevBuf x, d_row_off, d_seed, count, nan, off, idx(DevBuf::Growth::kQuarterMore), w(DevBuf::Growth::kQuarterMore);
  d_row_off.Upload(row_off, (size_t)(n_utts + 1) * 4, "copy row offsets");
  if (draws) d_seed.Upload(utt_seed, (size_t)n_utts * 8, "copy utterance seeds");
  count.Alloc((size_t)budget * 4);
  nan.Alloc((size_t)budget * 4);
  off.Alloc((size_t)(budget + 1) * 4);
  std::vector<int32_t> h_off, h_nan;
  EventTimer tm(timed);
  for (int64_t r0 = 0; r0 < rows; r0 += budget) {
    const int64_t n = std::min(budget, rows - r0);
    x.Upload(logprobs + (size_t)r0 * cols, (size_t)n * cols * 4, "copy log-probabilities");
    LogprobPostArgs a;
    memset(&a, 0, sizeof a);
    a.x = x.as<float>();
    a.row0 = r0;
    a.rows = (int)n;
    a.cols = cols;
    a.row_off = d_row_off.as<int32_t>();
    a.utt_seed = d_seed.as<uint64_t>();
    a.n_utts = n_utts;
    a.min_post = min_post;
    a.random_prune = random_prune ? 1 : 0;
    a.count = count.as<int32_t>();
    a.nan = nan.as<int32_t>();
    a.off = off.as<int32_t>();
    tm.Start();
    Check(launch_logprob_post_count(a, nullptr), "logprob_post_count launch");
    out->ms[0] += tm.Stop();
    tm.Start();
    Check(launch_logprob_post_scan(a, nullptr), "logprob_post_scan launch");
    out->ms[1] += tm.Stop();
    h_off.resize((size_t)n + 1);
    h_nan.resize((size_t)n);
    off.Download(h_off.data(), (size_t)(n + 1) * 4, "copy the pair offsets");
    nan.Download(h_nan.data(), (size_t)n * 4, "copy the NaN counts");
    const int64_t base = out->off[(size_t)r0], pairs = h_off[(size_t)n];
    for (int64_t i = 1; i <= n; ++i) out->off[(size_t)(r0 + i)] = base + h_off[(size_t)i];
    for (int32_t v : h_nan) out->num_nan += v;
    if (pairs == 0) continue;
    idx.Reserve((size_t)pairs * 4);
    w.Reserve((size_t)pairs * 4);
    a.idx = idx.as<int32_t>();
    a.w = w.as<float>();
    tm.Start();
    Check(launch_logprob_post_write(a, nullptr), "logprob_post_write launch");
    out->ms[2] += tm.Stop();
    out->idx.resize((size_t)(base + pairs));
    out->w.resize((size_t)(base + pairs));
    idx.Download(out->idx.data() + base, (size_t)pairs * 4, "copy the posterior indices");
    w.Download(out->w.data() + base, (size_t)pairs * 4, "copy the posteriors");
  }
}

float DeviceCopyMs(int device, size_t bytes, int reps) {
  UseDevice(device, kWhoNeeds);
  DevBuf src(bytes), dst(bytes);
  Check(hipMemset(src.p, 0, bytes), "hipMemset");
  EventTimer tm(true);
  float best = 0.f;
  BestOfReps(reps, 1, &best, [&](int, float* ms) {
    tm.Start();
    Check(hipMemcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
    *ms = tm.Stop();
  });
  return best;
}

void FgmmInitFromAccs(const FgmmAccs& accs, bool remove_low_count_gaussians, FullGmmData* model, FgmmInitResult* res) {
  *res = FgmmInitResult();
  const int all = kFgmmFlagMeans | kFgmmFlagVariances | kFgmmFlagWeights;
  if ((accs.flags & all) != all || !accs.full) throw KioError("the accumulators must carry the means, the covariances and the weights (update flags mvw)");
  const int G = accs.num_gauss, D = accs.dim;
  if (G < 1 || D < 1) throw KioError("the accumulators are empty");
  std::vector<char> bad((size_t)G, 0);
  std::vector<std::string> why((size_t)G);
  FullGmmData& m = *model;
  m = FullGmmData();
  m.num_gauss = G;
  m.dim = D;
  m.weights.assign((size_t)G, 0.f);
  m.means_invcovars.assign((size_t)G * D, 0.f);
  m.inv_covars.assign((size_t)G * Tri(D), 0.f);
  std::vector<double> mu((size_t)D), c((size_t)D * D), inv((size_t)D * D);
  res->inv_covars64.assign((size_t)G * Tri(D), 0.0);
  for (int g = 0; g < G; ++g) {
    float* ic = m.inv_covars.data() + (size_t)g * Tri(D);
    const double occ = accs.occ[g];
    bool ok = occ > 0.0;
    if (!ok) why[g] = "its occupancy is " + std::to_string(occ);
    if (ok) {
      const double* cov = accs.second.data() + (size_t)g * Tri(D);
      for (int d = 0; d < D; ++d) mu[d] = accs.mean[(size_t)g * D + d] / occ;
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) c[(size_t)i * D + j] = c[(size_t)j * D + i] = cov[Tri(i) + j] / occ - mu[i] * mu[j];
      ok = InvertSymmetric(D, c.data(), inv.data());
      if (!ok) why[g] = "its covariance is not positive definite and cannot be inverted";
    }
    if (!ok) {   // a stand-in until the Gaussian is removed: the unit covariance around 0, no weight
      bad[g] = 1;
      for (int d = 0; d < D; ++d) ic[Tri(d) + d] = 1.f;
      continue;
    }
    for (int i = 0; i < D; ++i) {
      for (int j = 0; j <= i; ++j) {
        res->inv_covars64[(size_t)g * Tri(D) + Tri(i) + j] = inv[(size_t)i * D + j];
        ic[Tri(i) + j] = (float)inv[(size_t)i * D + j];
      }
      double s = 0.0;
      for (int j = 0; j < D; ++j) s += inv[(size_t)i * D + j] * mu[j];
      m.means_invcovars[(size_t)g * D + i] = (float)s;
    }
  }
  // the weights of the Gaussians that are good so far, then the gconsts, which may find more; at most two rounds
  auto weights = [&] {
    double sum = 0.0;
    for (int g = 0; g < G; ++g)
      if (!bad[g]) sum += accs.occ[g];
    for (int g = 0; g < G; ++g) m.weights[g] = bad[g] ? 0.f : (float)(accs.occ[g] / sum);
  };
  weights();
  ComputeGconsts(&m);
  for (int g = 0; g < G; ++g)
    if (!bad[g] && !std::isfinite(m.gconsts[g])) {
      bad[g] = 1;
      why[g] = "its gconst is not finite";
      ++res->bad_gconsts;
    }
  int left = 0;
  for (int g = 0; g < G; ++g) {
    if (!bad[g]) {
      ++left;
      continue;
    }
    if (!remove_low_count_gaussians)
      throw KioError("Gaussian " + std::to_string(g) + " cannot be initialised: " + why[g] + " (and --remove-low-count-gaussians=false)");
    res->warnings.push_back("Removing Gaussian " + std::to_string(g) + ": " + why[g]);
    res->removed.push_back(g);
  }
  if (left == 0) throw KioError("no Gaussian of the " + std::to_string(G) + " can be initialised from these statistics");
  if (res->removed.empty()) return;
  weights();
  RemoveGmmRows(bad, 1, &m.weights);
  RemoveGmmRows(bad, (size_t)D, &m.means_invcovars);
  RemoveGmmRows(bad, Tri(D), &m.inv_covars);
  m.num_gauss = left;
  ComputeGconsts(&m);
}

}  // namespace xv
