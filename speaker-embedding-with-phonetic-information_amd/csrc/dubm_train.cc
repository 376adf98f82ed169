#include "dubm_train.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <set>

#include "device.h"
#include "dubm_train_kernels.h"
#include "gmm_sparse_acc.h"
#include "ivex_train.h"
#include "ubm_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "diagonal UBM training needs";

}  // namespace

uint64_t DgmmDrawA(uint64_t seed, uint64_t e) { return Mix53(seed, 2 * e); }
uint64_t DgmmDrawB(uint64_t seed, uint64_t e) { return Mix53(seed, 2 * e + 1); }
double DgmmGauss(uint64_t seed, uint64_t e) {
  const double two_pi = 6.283185307179586476925286766559;
  const double u1 = ((double)DgmmDrawA(seed, e) + 1.0) / 9007199254740992.0, u2 = (double)DgmmDrawB(seed, e) / 9007199254740992.0;
  return sqrt(-2.0 * log(u1)) * cos(two_pi * u2);
}

// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

double MlObjective(const DgmmAccs& a, const DiagGmmData& m) {
  const size_t G = (size_t)m.num_gauss, D = (size_t)m.dim;
  double obj = 0.0;
  for (size_t g = 0; g < G; ++g) obj += a.occ[g] * (double)m.gconsts[g];
  if (a.flags & kFgmmFlagMeans)
    for (size_t i = 0; i < G * D; ++i) obj += a.mean[i] * (double)m.means_invvars[i];
  if (a.flags & kFgmmFlagVariances) {
    double q = 0.0;
    for (size_t i = 0; i < G * D; ++i) q += a.second[i] * (double)m.inv_vars[i];
    obj -= 0.5 * q;
  }
  return obj;
}

}  // namespace

void DgmmEst(const DgmmAccs& accs, int update_flags, const DgmmEstOptions& o, DiagGmmData* model, DgmmEstResult* res) {
  const int D = model->dim;
  const bool upd_m = update_flags & kFgmmFlagMeans, upd_v = update_flags & kFgmmFlagVariances;
  const bool has_m = accs.flags & kFgmmFlagMeans, has_v = accs.flags & kFgmmFlagVariances;
  std::vector<double> mu((size_t)D), var((size_t)D);
  GmmEstKind k;
  k.num_gauss = &model->num_gauss;
  k.dim = D;
  k.weights = &model->weights;
  k.rows = {{&model->means_invvars, (size_t)D}, {&model->inv_vars, (size_t)D}};
  k.min_gaussian_weight = o.min_gaussian_weight;
  k.min_gaussian_occupancy = o.min_gaussian_occupancy;
  k.remove_low_count_gaussians = o.remove_low_count_gaussians;
  k.gconsts_before = true;
  k.gconsts = [&] { ComputeGconsts(model); };
  k.objective = [&] { return MlObjective(accs, *model); };
  k.update = [&](int g, double occ) {
    if (!has_m) return;
    float* iv = model->inv_vars.data() + (size_t)g * D;
    float* mi = model->means_invvars.data() + (size_t)g * D;
    int floored = 0;
    for (int d = 0; d < D; ++d) {
      const double mu_old = (double)mi[d] / (double)iv[d];
      mu[d] = accs.mean[(size_t)g * D + d] / occ;
      if (has_v) {
        double v = accs.second[(size_t)g * D + d] / occ - mu[d] * mu[d];
        if (!upd_m) v += (mu[d] - mu_old) * (mu[d] - mu_old);
        if (v < o.min_variance) {
          v = o.min_variance;
          ++floored;
        }
        var[d] = v;
      }
      if (!upd_m) mu[d] = mu_old;
    }
    if (floored) {
      res->floored_elements += floored;
      ++res->floored_gauss;
    }
    if (!upd_m && !upd_v) return;
    for (int d = 0; d < D; ++d) {
      const double inv = upd_v ? 1.0 / var[d] : (double)iv[d];
      if (upd_v) iv[d] = (float)inv;
      mi[d] = (float)(mu[d] * inv);
    }
  };
  GmmEst(accs, update_flags, k, res);
}

void DgmmSplit(DiagGmmData* m, int target, double perturb, uint64_t seed, uint64_t stream, std::vector<int32_t>* split_of) {
  const int D = m->dim;
  if (split_of) split_of->clear();
  if (target <= m->num_gauss) return;
  if (target > (1 << 20)) throw KioError("a split to more than 2^20 Gaussians");
  while (m->num_gauss < target) {
    const int cur = m->num_gauss;
    int best = 0;
    for (int g = 1; g < cur; ++g)
      if (m->weights[g] > m->weights[best]) best = g;
    const float half = m->weights[best] / 2.f;
    m->weights[best] = half;
    m->weights.push_back(half);
    m->inv_vars.resize((size_t)(cur + 1) * D);
    m->means_invvars.resize((size_t)(cur + 1) * D);
    for (int d = 0; d < D; ++d) {
      const float iv = m->inv_vars[(size_t)best * D + d], mi = m->means_invvars[(size_t)best * D + d];
      const double r = DgmmGauss(seed, kDgmmEntrySplit + (stream << 36) + (uint64_t)cur * D + d) * sqrt((double)iv);
      m->inv_vars[(size_t)cur * D + d] = iv;
      m->means_invvars[(size_t)cur * D + d] = (float)((double)mi + perturb * r);
      m->means_invvars[(size_t)best * D + d] = (float)((double)mi - perturb * r);
    }
    if (split_of) split_of->push_back(best);
    m->num_gauss = cur + 1;
  }
  ComputeGconsts(m);
}

void DgmmFrameSampler::Add(const float* row) {
  ++num_read;
  if (num_read <= num_frames) {
    kept.insert(kept.end(), row, row + dim);
    return;
  }
  const uint64_t e = kDgmmEntrySample + (uint64_t)num_read;
  if ((double)DgmmDrawA(seed, e) / 9007199254740992.0 < (double)num_frames / (double)num_read) {
    const size_t slot = (size_t)(DgmmDrawB(seed, e) % (uint64_t)num_frames);
    std::copy(row, row + dim, kept.begin() + slot * dim);
  }
}

void DgmmInitFromFrames(const float* feats, int64_t rows, int dim, int num_gauss, uint64_t seed, DiagGmmData* out) {
  if (num_gauss < 1 || dim < 1 || rows < 0) throw KioError("GMM initialisation: bad argument");
  if (rows < 10 * (int64_t)num_gauss)
    throw KioError("Too few frames to train on: " + std::to_string(rows) + " frames for " + std::to_string(num_gauss) + " Gaussians (10 per Gaussian are needed)");
  std::vector<double> mean((size_t)dim, 0.0), var((size_t)dim, 0.0);
  for (int64_t t = 0; t < rows; ++t)
    for (int d = 0; d < dim; ++d) {
      const double x = (double)feats[(size_t)t * dim + d];
      mean[d] += x;
      var[d] += x * x;
    }
  for (int d = 0; d < dim; ++d) {
    mean[d] /= (double)rows;
    var[d] = var[d] / (double)rows - mean[d] * mean[d];
    if (!(var[d] > 0.0)) throw KioError("Features do not have positive variance: dimension " + std::to_string(d) + " has " + std::to_string(var[d]));
  }
  *out = DiagGmmData();
  out->num_gauss = num_gauss;
  out->dim = dim;
  out->weights.assign((size_t)num_gauss, (float)(1.0 / num_gauss));
  out->inv_vars.resize((size_t)num_gauss * dim);
  out->means_invvars.resize((size_t)num_gauss * dim);
  std::set<int64_t> used;
  uint64_t attempt = 0;
  for (int g = 0; g < num_gauss; ++g) {
    int64_t f;
    do {
      f = (int64_t)(DgmmDrawA(seed, kDgmmEntryInit + attempt++) % (uint64_t)rows);
    } while (!used.insert(f).second);
    for (int d = 0; d < dim; ++d) {
      const double inv = 1.0 / var[d];
      out->inv_vars[(size_t)g * dim + d] = (float)inv;
      out->means_invvars[(size_t)g * dim + d] = (float)((double)feats[(size_t)f * dim + d] * inv);
    }
  }
  ComputeGconsts(out);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct DgmmAccumulator::Impl {
  GmmSparseAcc acc;                                             // the running accumulators and the sparse path
  DevBuf gselect;                                               // DgmmAccAddGselect's input
  DevBuf ll, count, pidx, post, logsum, slot_post;              // the sparse E-step
  DevBuf dense_post;
  DevBuf resident;                                              // DgmmAccSetFrames
  int64_t resident_rows = 0;
};

DgmmAccumulator::~DgmmAccumulator() {}
int DgmmAccumulator::num_gauss() const { return impl_->acc.num_gauss; }
int DgmmAccumulator::dim() const { return impl_->acc.dim; }
int DgmmAccumulator::flags() const { return impl_->acc.flags; }

DgmmAccumulator* DgmmAccCreate(int device, int num_gauss, int dim, int flags) {
  if (num_gauss < 1 || dim < 1 || flags < 0 || flags > 7) throw KioError("dgmm accumulator: bad argument");
  if (dim > kDgmmMaxDim)
    throw KioError("the dimension " + std::to_string(dim) + " is above the accumulation kernels' limit of " + std::to_string(kDgmmMaxDim));
  if (num_gauss > (1 << 20)) throw KioError("the model has more than 2^20 components");
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<DgmmAccumulator> a(new DgmmAccumulator);
  a->impl_.reset(new DgmmAccumulator::Impl);
  GmmSparseAcc& A = a->impl_->acc;
  A.device = device;
  A.dim = dim;
  A.flags = AugmentGmmFlags(flags);
  A.second_width = (size_t)dim;
  A.who_needs = kWhoNeeds;
  DgmmAccReset(a.get(), num_gauss);
  return a.release();
}

void DgmmAccReset(DgmmAccumulator* acc, int num_gauss) {
  if (num_gauss < 1 || num_gauss > (1 << 20)) throw KioError("dgmm accumulator: bad number of components");
  acc->impl_->acc.Reset(num_gauss);
}

namespace {

using Impl = DgmmAccumulator::Impl;

// the work items, the partial sums and the reduction on the pairs that A.Sort bucketed.  a: feats, rows, pairs, pair_frame / n, pair_w.
float RunSparseAcc(GmmSparseAcc& A, FgmmAccArgs a, bool timed) {
  a.sorted = A.sort.sorted.as<int32_t>();
  a.bucket_start = A.sort.start.as<int32_t>();
  return A.Accumulate(
      a,
      [](int64_t bound, size_t) {
        if (bound >= INT32_MAX) throw KioError("dgmm accumulate: too many pairs in one call");
      },
      launch_dgmm_acc, "dgmm_acc launch", timed);
}

DgmmModelArgs ModelArgs(const Impl& I, const UbmModel& diag, const char* who) {
  const UbmDiagView v = UbmDiagArrays(diag);
  if (v.num_gauss != I.acc.num_gauss || v.dim != I.acc.dim)
    throw KioError(std::string(who) + ": the model has " + std::to_string(v.num_gauss) + " components of dimension " + std::to_string(v.dim) +
                   ", the accumulators " + std::to_string(I.acc.num_gauss) + " of dimension " + std::to_string(I.acc.dim));
  if (v.device != I.acc.device) throw KioError(std::string(who) + ": the model and the accumulators are on different devices");
  DgmmModelArgs m;
  m.dim = v.dim;
  m.num_gauss = v.num_gauss;
  m.gauss_pad = v.gauss_pad;
  m.m_t = v.m_t;
  m.v_t = v.v_t;
  m.gconst = v.gconst;
  return m;
}

// the dense accumulation and the reduction on frames that are on the device
void RunDense(Impl& I, DgmmDenseArgs a, float* ms_acc, float* ms_reduce) {
  a.num_chunks = (int)((a.rows + kDgmmDenseFrameChunk - 1) / kDgmmDenseFrameChunk);
  const size_t partial_bytes = (size_t)I.acc.num_gauss * a.num_chunks * (1 + 2 * I.acc.dim) * 8;
  if (partial_bytes > ((size_t)8 << 30))
    throw KioError("dgmm dense accumulate: " + std::to_string(a.rows) + " frames on " + std::to_string(I.acc.num_gauss) + " Gaussians of dimension " +
                   std::to_string(I.acc.dim) + " need " + std::to_string(partial_bytes >> 20) + " MiB of partial sums; the limit of one call is 8192 MiB");
  I.acc.partial.Reserve(partial_bytes);
  a.partial = I.acc.partial.as<double>();
  const bool timed = ms_acc != nullptr;
  EventTimer tm(timed, 3);
  tm.Mark();
  Check(launch_dgmm_dense_acc(a, nullptr), "dgmm_dense_acc launch");
  tm.Mark();
  DgmmReduceArgs r;
  memset(&r, 0, sizeof r);
  r.dim = I.acc.dim;
  r.num_gauss = I.acc.num_gauss;
  r.flags = I.acc.flags;
  r.num_chunks = a.num_chunks;
  r.partial = a.partial;
  r.occ = I.acc.occ.as<double>();
  r.mean = I.acc.mean.as<double>();
  r.var = I.acc.second.as<double>();
  Check(launch_dgmm_acc_reduce(r, nullptr), "dgmm_acc_reduce launch");
  tm.Mark();
  if (timed) {
    *ms_acc = tm.Span(0);
    *ms_reduce = tm.Span(1);
  }
}

}  // namespace

void DgmmAccAdd(DgmmAccumulator* acc, const float* feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w,
                float* device_ms2) {
  if (device_ms2) device_ms2[0] = device_ms2[1] = 0.f;
  GmmSparseAcc& A = acc->impl_->acc;
  const int64_t pairs = A.UploadPairs("dgmm accumulate", feats, rows, post_off, post_idx, post_w);
  if (pairs == 0) return;
  const float ms_sort = A.Sort(A.idx.as<int32_t>(), pairs, device_ms2 != nullptr);
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = A.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = A.frame.as<int32_t>();
  a.n = 1;
  a.pair_w = A.w.as<float>();
  const float ms = RunSparseAcc(A, a, device_ms2 != nullptr);
  if (device_ms2) {
    device_ms2[0] = ms_sort;
    device_ms2[1] = ms;
  }
  Check(hipDeviceSynchronize(), "dgmm_acc");
}

void DgmmAccAddGselect(DgmmAccumulator* acc, const UbmModel& diag, const float* feats, int64_t rows, const int32_t* gselect, int n, float* loglikes,
                       float* logsum, float* device_ms4) {
  if (device_ms4) device_ms4[0] = device_ms4[1] = device_ms4[2] = device_ms4[3] = 0.f;
  Impl& I = *acc->impl_;
  if (rows < 0) throw KioError("dgmm accumulate: bad argument");
  DgmmSelArgs sel;
  memset(&sel, 0, sizeof sel);
  sel.model = ModelArgs(I, diag, "dgmm accumulate");
  if (n < 1 || n > kUbmMaxSelect)
    throw KioError("dgmm accumulate: " + std::to_string(n) + " selected Gaussians per frame; the device kernels take 1 to " + std::to_string(kUbmMaxSelect));
  if (rows == 0) return;
  if (!feats || !gselect || !logsum) throw KioError("dgmm accumulate: null buffer");
  if (rows * n >= INT32_MAX) throw KioError("dgmm accumulate: more than 2^31 pairs in one call");
  const int64_t pairs = rows * n;
  for (int64_t i = 0; i < pairs; ++i)
    if (gselect[i] < 0 || gselect[i] >= I.acc.num_gauss)
      throw KioError("dgmm accumulate: the selection names Gaussian " + std::to_string(gselect[i]) + "; the model has " + std::to_string(I.acc.num_gauss));
  UseDevice(I.acc.device, kWhoNeeds);
  const bool timed = device_ms4 != nullptr;
  I.acc.feats.Upload(feats, (size_t)rows * I.acc.dim * 4, "copy features");
  I.gselect.Upload(gselect, (size_t)pairs * 4, "copy the selection");
  I.ll.Reserve((size_t)pairs * 4);
  I.count.Reserve((size_t)rows * 4);
  I.pidx.Reserve((size_t)pairs * 4);
  I.post.Reserve((size_t)pairs * 4);
  I.slot_post.Reserve((size_t)pairs * 4);
  I.logsum.Reserve((size_t)rows * 4);
  // the pairs (frame, slot) are bucketed by their Gaussian: n = 1 over rows * n pairs is the same sort as n over rows frames
  const float ms_sort = I.acc.Sort(I.gselect.as<int32_t>(), pairs, timed);
  sel.feats = I.acc.feats.as<float>();
  sel.rows = rows;
  sel.n = n;
  sel.gselect = I.gselect.as<int32_t>();
  sel.ll = I.ll.as<float>();
  UbmFullArgs p;
  memset(&p, 0, sizeof p);
  p.rows = rows;
  p.dim = I.acc.dim;
  p.num_gauss = I.acc.num_gauss;
  p.n = n;
  p.gselect = I.gselect.as<int32_t>();
  p.bucket_start = I.acc.sort.start.as<int32_t>();
  p.sorted = I.acc.sort.sorted.as<int32_t>();
  p.ll = I.ll.as<float>();
  p.min_post = 0.f;
  p.out_count = I.count.as<int32_t>();
  p.out_idx = I.pidx.as<int32_t>();
  p.out_post = I.post.as<float>();
  p.out_logsum = I.logsum.as<float>();
  p.out_slot_post = I.slot_post.as<float>();
  EventTimer tm(timed, 3);
  tm.Mark();
  Check(launch_dgmm_sel_loglike(sel, nullptr), "dgmm_sel_loglike launch");
  tm.Mark();
  Check(launch_ubm_post(p, nullptr), "ubm_post launch");
  tm.Mark();
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = I.acc.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = nullptr;
  a.n = n;
  a.pair_w = I.slot_post.as<float>();
  const float ms = RunSparseAcc(I.acc, a, timed);
  if (timed) {
    device_ms4[0] = ms_sort;
    device_ms4[1] = tm.Span(0);
    device_ms4[2] = tm.Span(1);
    device_ms4[3] = ms;
  }
  I.logsum.Download(logsum, (size_t)rows * 4, "copy the log-sums");
  if (loglikes) I.ll.Download(loglikes, (size_t)pairs * 4, "copy the log-likelihoods");
}

void DgmmAccAddDensePost(DgmmAccumulator* acc, const float* feats, int64_t rows, const float* post) {
  Impl& I = *acc->impl_;
  if (rows < 0) throw KioError("dgmm dense accumulate: bad argument");
  if (rows == 0) return;
  if (!feats || !post) throw KioError("dgmm dense accumulate: null buffer");
  UseDevice(I.acc.device, kWhoNeeds);
  I.acc.feats.Upload(feats, (size_t)rows * I.acc.dim * 4, "copy features");
  I.dense_post.Upload(post, (size_t)rows * I.acc.num_gauss * 4, "copy the posteriors");
  DgmmDenseArgs a;
  memset(&a, 0, sizeof a);
  a.model.dim = I.acc.dim;
  a.model.num_gauss = I.acc.num_gauss;
  a.feats = I.acc.feats.as<float>();
  a.rows = rows;
  a.post = I.dense_post.as<float>();
  RunDense(I, a, nullptr, nullptr);
  Check(hipDeviceSynchronize(), "dgmm_dense_acc");
}

void DgmmAccSetFrames(DgmmAccumulator* acc, const float* feats, int64_t rows) {
  Impl& I = *acc->impl_;
  if (rows < 1 || !feats) throw KioError("dgmm dense accumulate: no frames");
  UseDevice(I.acc.device, kWhoNeeds);
  I.resident.Upload(feats, (size_t)rows * I.acc.dim * 4, "copy features");
  I.resident_rows = rows;
}

void DgmmAccAddDense(DgmmAccumulator* acc, const UbmModel& diag, const float* feats, int64_t rows, float* logsum, float* device_ms3) {
  if (device_ms3) device_ms3[0] = device_ms3[1] = device_ms3[2] = 0.f;
  Impl& I = *acc->impl_;
  if (rows < 0) throw KioError("dgmm dense accumulate: bad argument");
  DgmmDenseArgs a;
  memset(&a, 0, sizeof a);
  a.model = ModelArgs(I, diag, "dgmm dense accumulate");
  if (rows == 0) return;
  if (!feats && rows != I.resident_rows) throw KioError("dgmm dense accumulate: the frames on the device are not the " + std::to_string(rows) + " asked for");
  UseDevice(I.acc.device, kWhoNeeds);
  if (feats) I.acc.feats.Upload(feats, (size_t)rows * I.acc.dim * 4, "copy features");
  I.logsum.Reserve((size_t)rows * 4);
  a.feats = feats ? I.acc.feats.as<float>() : I.resident.as<float>();
  a.rows = rows;
  a.logsum = I.logsum.as<float>();
  EventTimer tm(device_ms3 != nullptr);
  tm.Start();
  Check(launch_dgmm_dense_logsum(a, nullptr), "dgmm_dense_logsum launch");
  if (device_ms3) device_ms3[0] = tm.Stop();
  RunDense(I, a, device_ms3 ? device_ms3 + 1 : nullptr, device_ms3 ? device_ms3 + 2 : nullptr);
  if (logsum) I.logsum.Download(logsum, (size_t)rows * 4, "copy the log-sums");
  else Check(hipDeviceSynchronize(), "dgmm_dense_acc");
}

void DgmmAccGet(const DgmmAccumulator& acc, double* occ, double* mean, double* var) {
  acc.impl_->acc.Get(occ, mean, var, "copy the variance accumulators");
}

}  // namespace xv
