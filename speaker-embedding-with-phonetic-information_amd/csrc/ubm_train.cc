#include "ubm_train.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "device.h"
#include "gmm_sparse_acc.h"
#include "plda.h"
#include "ubm_kernels.h"
#include "ubm_train_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "UBM training needs";

size_t Tri(int d) { return (size_t)d * (d + 1) / 2; }

// packed lower triangle (float, widened) -> symmetric [d][d]
void Unpack(const float* p, int d, double* a) {
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) a[(size_t)i * d + j] = a[(size_t)j * d + i] = (double)p[Tri(i) + j];
}

}  // namespace

void DiagGmmToFull(const DiagGmmData& diag, FullGmmData* full) {
  const int G = diag.num_gauss, D = diag.dim;
  *full = FullGmmData();
  full->num_gauss = G;
  full->dim = D;
  full->weights = diag.weights;
  full->means_invcovars = diag.means_invvars;
  full->inv_covars.assign((size_t)G * Tri(D), 0.f);
  for (int g = 0; g < G; ++g)
    for (int d = 0; d < D; ++d) full->inv_covars[(size_t)g * Tri(D) + Tri(d) + d] = diag.inv_vars[(size_t)g * D + d];
  ComputeGconsts(full);
}

// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// sum_g occ_g gconst_g + sum_g mean_acc_g . (Sigma^-1 mu)_g - 1/2 sum_g tr(cov_acc_g Sigma_g^-1)
double MlObjective(const FgmmAccs& a, const FullGmmData& m) {
  const int G = m.num_gauss, D = m.dim;
  double obj = 0.0;
  for (int g = 0; g < G; ++g) obj += a.occ[g] * (double)m.gconsts[g];
  if (a.flags & kFgmmFlagMeans)
    for (size_t i = 0; i < (size_t)G * D; ++i) obj += a.mean[i] * (double)m.means_invcovars[i];
  if (a.flags & kFgmmFlagVariances)
    for (int g = 0; g < G; ++g) {
      const double* c = a.second.data() + (size_t)g * Tri(D);
      const float* s = m.inv_covars.data() + (size_t)g * Tri(D);
      double tr = 0.0;   // the trace of the product of two symmetric matrices from their lower triangles
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) tr += (i == j ? 1.0 : 2.0) * c[Tri(i) + j] * (double)s[Tri(i) + j];
      obj -= 0.5 * tr;
    }
  return obj;
}

}  // namespace

void FgmmEst(const FgmmAccs& accs, int update_flags, const FgmmEstOptions& o, FullGmmData* model, FgmmEstResult* res) {
  const int D = model->dim;
  const bool upd_m = update_flags & kFgmmFlagMeans, upd_v = update_flags & kFgmmFlagVariances;
  std::vector<double> sig((size_t)D * D), inv((size_t)D * D), eig((size_t)D), U((size_t)D * D), mu((size_t)D), mu_old((size_t)D), diff((size_t)D);
  GmmEstKind k;
  k.num_gauss = &model->num_gauss;
  k.dim = D;
  k.weights = &model->weights;
  k.rows = {{&model->means_invcovars, (size_t)D}, {&model->inv_covars, Tri(D)}};
  k.min_gaussian_weight = o.min_gaussian_weight;
  k.min_gaussian_occupancy = o.min_gaussian_occupancy;
  k.remove_low_count_gaussians = o.remove_low_count_gaussians;
  k.gconsts = [&] { ComputeGconsts(model); };
  k.objective = [&] { return MlObjective(accs, *model); };
  k.update = [&](int g, double occ) {
    if (!upd_m && !upd_v) return;
    float* ic = model->inv_covars.data() + (size_t)g * Tri(D);
    float* lin = model->means_invcovars.data() + (size_t)g * D;
    for (int d = 0; d < D; ++d) mu[d] = accs.mean[(size_t)g * D + d] / occ;
    Unpack(ic, D, inv.data());   // the old Sigma^-1
    if (!upd_m) {                // the old mean = Sigma (Sigma^-1 mu)
      if (!InvertSymmetric(D, inv.data(), sig.data()))
        throw KioError("the inverse covariance of component " + std::to_string(g) + " is not positive definite: it cannot be inverted");
      for (int i = 0; i < D; ++i) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s += sig[(size_t)i * D + j] * (double)lin[j];
        mu_old[i] = s;
      }
    }
    if (upd_v) {
      const double* c = accs.second.data() + (size_t)g * Tri(D);
      for (int d = 0; d < D; ++d) diff[d] = upd_m ? 0.0 : mu_old[d] - mu[d];
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
          double v = c[Tri(i) + j] / occ - mu[i] * mu[j];
          if (!upd_m) v += diff[i] * diff[j];
          sig[(size_t)i * D + j] = sig[(size_t)j * D + i] = v;
        }
      SymmetricEig(D, sig.data(), eig.data(), U.data());
      double max_abs = 0.0;
      for (int d = 0; d < D; ++d) max_abs = std::max(max_abs, fabs(eig[d]));
      const double floor = std::max(o.variance_floor, max_abs / o.max_condition);
      int floored = 0;
      for (int d = 0; d < D; ++d)
        if (eig[d] < floor) {
          eig[d] = floor;
          ++floored;
        }
      if (floored) {
        res->floored_elements += floored;
        ++res->floored_gauss;
        for (int i = 0; i < D; ++i)
          for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k2 = 0; k2 < D; ++k2) v += U[(size_t)i * D + k2] * eig[k2] * U[(size_t)j * D + k2];
            sig[(size_t)i * D + j] = sig[(size_t)j * D + i] = v;
          }
      }
      if (!InvertSymmetric(D, sig.data(), inv.data()))
        throw KioError("the new covariance of component " + std::to_string(g) + " is not positive definite after flooring");
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) ic[Tri(i) + j] = (float)inv[(size_t)i * D + j];
    }
    const double* m_use = upd_m ? mu.data() : mu_old.data();
    for (int i = 0; i < D; ++i) {
      double s = 0.0;
      for (int j = 0; j < D; ++j) s += inv[(size_t)i * D + j] * m_use[j];
      lin[i] = (float)s;
    }
  };
  GmmEst(accs, update_flags, k, res);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct FgmmAccumulator::Impl {
  GmmSparseAcc acc;    // FgmmAccAdd sorts its pairs there
  UbmPostDevice post;  // FgmmAccAddGselect
};

FgmmAccumulator::~FgmmAccumulator() {}
int FgmmAccumulator::num_gauss() const { return impl_->acc.num_gauss; }
int FgmmAccumulator::dim() const { return impl_->acc.dim; }
int FgmmAccumulator::flags() const { return impl_->acc.flags; }

FgmmAccumulator* FgmmAccCreate(int device, int num_gauss, int dim, int flags) {
  if (num_gauss < 1 || dim < 1 || flags < 0 || flags > 7) throw KioError("fgmm accumulator: bad argument");
  if (dim > kFgmmAccMaxDim)
    throw KioError("the dimension " + std::to_string(dim) + " is above the accumulation kernel's limit of " + std::to_string(kFgmmAccMaxDim));
  if (num_gauss > (1 << 20)) throw KioError("the model has more than 2^20 components");
  std::unique_ptr<FgmmAccumulator> a(new FgmmAccumulator);
  a->impl_.reset(new FgmmAccumulator::Impl);
  GmmSparseAcc& A = a->impl_->acc;
  A.device = device;
  A.dim = dim;
  A.flags = AugmentGmmFlags(flags);
  A.second_width = Tri(dim);
  A.who_needs = kWhoNeeds;
  A.Reset(num_gauss);
  return a.release();
}

namespace {

// the work items, then the accumulation.  a: everything but item_start, num_items, partial and the accumulators.  Returns the ms.
float RunAcc(GmmSparseAcc& A, const FgmmAccArgs& a, bool timed) {
  return A.Accumulate(
      a,
      [&](int64_t bound, size_t partial_bytes) {
        if (bound >= INT32_MAX || partial_bytes > ((size_t)8 << 30))
          throw KioError("fgmm accumulate: " + std::to_string(a.pairs) + " pairs on " + std::to_string(A.num_gauss) + " Gaussians of dimension " +
                         std::to_string(A.dim) + " need " + std::to_string(partial_bytes >> 20) + " MiB of partial sums; the limit of one call is 8192 MiB");
      },
      launch_fgmm_acc, "fgmm_acc launch", timed);
}

}  // namespace

void FgmmAccAdd(FgmmAccumulator* acc, const float* feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w,
                float* device_ms2) {
  if (device_ms2) device_ms2[0] = device_ms2[1] = 0.f;
  GmmSparseAcc& A = acc->impl_->acc;
  const int64_t pairs = A.UploadPairs("fgmm accumulate", feats, rows, post_off, post_idx, post_w);
  if (pairs == 0) return;
  const float ms_sort = A.Sort(A.idx.as<int32_t>(), pairs, device_ms2 != nullptr);
  if (device_ms2) device_ms2[0] = ms_sort;
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = A.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = A.frame.as<int32_t>();
  a.n = 1;
  a.pair_w = A.w.as<float>();
  a.sorted = A.sort.sorted.as<int32_t>();
  a.bucket_start = A.sort.start.as<int32_t>();
  const float ms = RunAcc(A, a, device_ms2 != nullptr);
  if (device_ms2) device_ms2[1] = ms;
  Check(hipDeviceSynchronize(), "fgmm_acc");
}

void FgmmAccAddGselect(FgmmAccumulator* acc, const UbmModel& full, const float* feats, int64_t rows, const int32_t* gselect, int n, float* logsum,
                       float* device_ms4) {
  if (device_ms4) device_ms4[0] = device_ms4[1] = device_ms4[2] = device_ms4[3] = 0.f;
  FgmmAccumulator::Impl& I = *acc->impl_;
  GmmSparseAcc& A = I.acc;
  if (rows < 0) throw KioError("fgmm accumulate: bad argument");
  if (full.full() && (full.num_gauss() != A.num_gauss || full.dim() != A.dim))
    throw KioError("fgmm accumulate: the model has " + std::to_string(full.num_gauss()) + " components of dimension " + std::to_string(full.dim()) +
                   ", the accumulators " + std::to_string(A.num_gauss) + " of dimension " + std::to_string(A.dim));
  if (full.device() != A.device) throw KioError("fgmm accumulate: the model and the accumulators are on different devices");
  CheckUbmSelection("fgmm accumulate", full, gselect, rows, n);
  if (rows == 0) return;
  if (!feats || !logsum) throw KioError("fgmm accumulate: null buffer");
  if (rows * n >= INT32_MAX) throw KioError("fgmm accumulate: more than 2^31 pairs in one call");
  UseDevice(A.device, kWhoNeeds);
  I.post.Run(full, feats, gselect, rows, n, 0.f, true, device_ms4);
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = I.post.feats.as<float>();
  a.rows = rows;
  a.pairs = rows * n;
  a.pair_frame = nullptr;
  a.n = n;
  a.pair_w = I.post.slot_post.as<float>();
  a.sorted = I.post.sort.sorted.as<int32_t>();
  a.bucket_start = I.post.sort.start.as<int32_t>();
  const float ms = RunAcc(A, a, device_ms4 != nullptr);
  if (device_ms4) device_ms4[3] = ms;
  I.post.logsum.Download(logsum, (size_t)rows * 4, "copy the log-sums");
}

void FgmmAccGet(const FgmmAccumulator& acc, double* occ, double* mean, double* cov) {
  acc.impl_->acc.Get(occ, mean, cov, "copy the covariance accumulators");
}

}  // namespace xv
