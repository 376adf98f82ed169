#include "ubm_train.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <sstream>

#include "device.h"
#include "plda.h"
#include "ubm_kernels.h"
#include "ubm_train_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "UBM training needs";

size_t Tri(int d) { return (size_t)d * (d + 1) / 2; }

std::string FlagLetters(int flags) {
  std::string s;
  if (flags & kFgmmFlagMeans) s += 'm';
  if (flags & kFgmmFlagVariances) s += 'v';
  if (flags & kFgmmFlagWeights) s += 'w';
  return s;
}

// packed lower triangle (float, widened) -> symmetric [d][d]
void Unpack(const float* p, int d, double* a) {
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) a[(size_t)i * d + j] = a[(size_t)j * d + i] = (double)p[Tri(i) + j];
}

}  // namespace

int ParseGmmFlags(const std::string& letters) {
  int flags = 0;
  for (char c : letters) {
    if (c == 'm') flags |= kFgmmFlagMeans;
    else if (c == 'v') flags |= kFgmmFlagVariances;
    else if (c == 'w') flags |= kFgmmFlagWeights;
    else throw KioError("Invalid element '" + std::string(1, c) + "' of the update flags '" + letters + "': they are made of m, v and w");
  }
  return flags;
}

int AugmentGmmFlags(int flags) {
  if (flags & kFgmmFlagVariances) flags |= kFgmmFlagMeans;
  if (flags & kFgmmFlagMeans) flags |= kFgmmFlagWeights;
  return flags;
}

void FgmmAccs::Init(int g, int d, int f) {
  if (g < 1 || d < 1 || f < 0 || f > 7) throw KioError("GMM accumulators: bad shape or flags");
  num_gauss = g;
  dim = d;
  flags = AugmentGmmFlags(f);
  occ.assign((size_t)g, 0.0);
  mean.assign((size_t)g * d, 0.0);
  cov.assign((size_t)g * Tri(d), 0.0);
}

void ReadFgmmAccs(Input& in, bool binary, bool add, FgmmAccs* a) {
  ExpectToken(in, binary, "<GMMACCS>");
  ExpectToken(in, binary, "<VECSIZE>");
  const int dim = ReadInt32(in, binary);
  ExpectToken(in, binary, "<NUMCOMPONENTS>");
  const int G = ReadInt32(in, binary);
  ExpectToken(in, binary, "<FLAGS>");
  int flags;
  if (binary) {
    if (in.Get() != 2) throw KioError("expected uint16 (size byte 2) in " + in.Name());
    uint16_t v;
    in.Read(&v, 2);
    flags = v;
  } else {
    flags = ReadInt32(in, false);
  }
  if (dim < 1 || G < 1 || flags < 0 || flags > 7 || AugmentGmmFlags(flags) != flags)
    throw KioError("GMM accumulators with dimension " + std::to_string(dim) + ", " + std::to_string(G) + " components and flags " + std::to_string(flags));
  if (!add) a->Init(G, dim, flags);
  else if (a->dim != dim || a->num_gauss != G || a->flags != flags)
    throw KioError("the accumulators of " + in.Name() + " (dimension " + std::to_string(dim) + ", " + std::to_string(G) + " components, flags " +
                   FlagLetters(flags) + ") cannot be added to ones of dimension " + std::to_string(a->dim) + ", " + std::to_string(a->num_gauss) +
                   " components, flags " + FlagLetters(a->flags));
  ExpectToken(in, binary, "<OCCUPANCY>");
  std::vector<float> v;
  ReadVector(in, binary, &v);
  if ((int)v.size() != G) throw KioError("<OCCUPANCY> has " + std::to_string(v.size()) + " values for " + std::to_string(G) + " components");
  for (int g = 0; g < G; ++g) a->occ[g] += (double)v[g];
  ExpectToken(in, binary, "<MEANACCS>");
  Matrix m;
  ReadMatrix(in, binary, &m);
  if (m.rows != G || m.cols != dim) throw KioError("<MEANACCS> is " + std::to_string(m.rows) + " x " + std::to_string(m.cols));
  for (size_t i = 0; i < (size_t)G * dim; ++i) a->mean[i] += (double)m.Data()[i];
  if (flags & kFgmmFlagVariances) {
    ExpectToken(in, binary, "<FULLVARACCS>");
    for (int g = 0; g < G; ++g) {
      v.clear();
      if (ReadPackedMatrix(in, binary, &v) != dim) throw KioError("a covariance accumulator does not have the dimension " + std::to_string(dim));
      double* c = a->cov.data() + (size_t)g * Tri(dim);
      for (size_t i = 0; i < v.size(); ++i) c[i] += (double)v[i];
    }
  }
  ExpectToken(in, binary, "</GMMACCS>");
}

void ReadFgmmAccsFile(const std::string& rxfilename, bool add, FgmmAccs* a) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ReadFgmmAccs(in, binary, add, a);
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
}

void WriteFgmmAccsFile(const std::string& wxfilename, bool binary, const FgmmAccs& a) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteToken(out, binary, "<GMMACCS>");
  WriteToken(out, binary, "<VECSIZE>");
  WriteInt32(out, binary, a.dim);
  WriteToken(out, binary, "<NUMCOMPONENTS>");
  WriteInt32(out, binary, a.num_gauss);
  WriteToken(out, binary, "<FLAGS>");
  if (binary) {
    const uint16_t v = (uint16_t)a.flags;
    out.Put((char)2);
    out.Write(&v, 2);
  } else {
    WriteInt32(out, false, a.flags);
  }
  std::vector<float> f(a.occ.begin(), a.occ.end());   // the one rounding
  WriteToken(out, binary, "<OCCUPANCY>");
  WriteVector(out, binary, f.data(), a.num_gauss);
  Matrix m;
  m.rows = a.num_gauss;
  m.cols = a.dim;
  m.data.assign(a.mean.begin(), a.mean.end());
  WriteToken(out, binary, "<MEANACCS>");
  WriteMatrix(out, binary, m);
  if (a.flags & kFgmmFlagVariances) {
    WriteToken(out, binary, "<FULLVARACCS>");
    for (int g = 0; g < a.num_gauss; ++g) {
      f.assign(a.cov.begin() + (size_t)g * Tri(a.dim), a.cov.begin() + (size_t)(g + 1) * Tri(a.dim));
      WritePackedMatrix(out, binary, f.data(), a.dim);
    }
  }
  WriteToken(out, binary, "</GMMACCS>");
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

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
      const double* c = a.cov.data() + (size_t)g * Tri(D);
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
  const int G = model->num_gauss, D = model->dim;
  if (accs.num_gauss != G || accs.dim != D)
    throw KioError("the accumulators (" + std::to_string(accs.num_gauss) + " components of dimension " + std::to_string(accs.dim) + ") are not the model's (" +
                   std::to_string(G) + " of dimension " + std::to_string(D) + ")");
  if (update_flags & ~accs.flags)
    throw KioError("the update flags '" + FlagLetters(update_flags) + "' name statistics that the accumulators (flags '" + FlagLetters(accs.flags) + "') do not have");
  *res = FgmmEstResult();
  const bool upd_m = update_flags & kFgmmFlagMeans, upd_v = update_flags & kFgmmFlagVariances, upd_w = update_flags & kFgmmFlagWeights;
  res->objf_before = MlObjective(accs, *model);
  double occ_sum = 0.0;
  for (int g = 0; g < G; ++g) occ_sum += accs.occ[g];
  res->count = occ_sum;
  std::vector<double> w((size_t)G), sig((size_t)D * D), inv((size_t)D * D), eig((size_t)D), U((size_t)D * D), mu((size_t)D), mu_old((size_t)D), diff((size_t)D);
  std::vector<char> remove((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    const double occ = accs.occ[g];
    const double prob = occ_sum > 0.0 ? occ / occ_sum : 1.0 / G;
    if (occ > o.min_gaussian_occupancy && prob > o.min_gaussian_weight) {
      w[g] = prob;
      if (!upd_m && !upd_v) continue;
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
        const double* c = accs.cov.data() + (size_t)g * Tri(D);
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
              for (int k = 0; k < D; ++k) v += U[(size_t)i * D + k] * eig[k] * U[(size_t)j * D + k];
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
    } else if (o.remove_low_count_gaussians && (int)res->removed.size() < G - 1) {
      std::ostringstream msg;
      msg << "Too little data - removing Gaussian (weight " << prob << ", occupation count " << occ << ", vector size " << D << ")";
      res->warnings.push_back(msg.str());
      res->removed.push_back(g);
      remove[g] = 1;
      w[g] = (double)model->weights[g];   // until it is taken out it counts with its old weight
    } else {
      std::ostringstream msg;
      msg << "Gaussian has too little data but not removing it because "
          << (o.remove_low_count_gaussians ? "it is the last Gaussian: i = " : "remove-low-count-gaussians == false: i = ") << g << ", occ = " << occ
          << ", weight = " << prob;
      res->warnings.push_back(msg.str());
      w[g] = std::max(prob, o.min_gaussian_weight);
    }
  }
  if (upd_w) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += w[g];
    for (int g = 0; g < G; ++g) model->weights[g] = (float)(w[g] / sum);
  }
  ComputeGconsts(model);
  res->objf_after = MlObjective(accs, *model);
  if (!res->removed.empty()) {
    FullGmmData out;
    out.dim = D;
    double sum = 0.0;
    for (int g = 0; g < G; ++g)
      if (!remove[g]) sum += (double)model->weights[g];
    for (int g = 0; g < G; ++g) {
      if (remove[g]) continue;
      ++out.num_gauss;
      out.weights.push_back((float)((double)model->weights[g] / sum));
      out.means_invcovars.insert(out.means_invcovars.end(), model->means_invcovars.begin() + (size_t)g * D, model->means_invcovars.begin() + (size_t)(g + 1) * D);
      out.inv_covars.insert(out.inv_covars.end(), model->inv_covars.begin() + (size_t)g * Tri(D), model->inv_covars.begin() + (size_t)(g + 1) * Tri(D));
    }
    ComputeGconsts(&out);
    *model = out;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct FgmmAccumulator::Impl {
  int device = 0, num_gauss = 0, dim = 0, flags = 0;
  DevBuf occ, mean, cov;                                      // the running accumulators
  DevBuf feats, idx, w, frame, rank, hist, start, sorted;     // FgmmAccAdd's pairs and their sort
  DevBuf item_start, partial;
  UbmPostDevice post;                                         // FgmmAccAddGselect
};

FgmmAccumulator::~FgmmAccumulator() {}
int FgmmAccumulator::num_gauss() const { return impl_->num_gauss; }
int FgmmAccumulator::dim() const { return impl_->dim; }
int FgmmAccumulator::flags() const { return impl_->flags; }

FgmmAccumulator* FgmmAccCreate(int device, int num_gauss, int dim, int flags) {
  if (num_gauss < 1 || dim < 1 || flags < 0 || flags > 7) throw KioError("fgmm accumulator: bad argument");
  if (dim > kFgmmAccMaxDim)
    throw KioError("the dimension " + std::to_string(dim) + " is above the accumulation kernel's limit of " + std::to_string(kFgmmAccMaxDim));
  if (num_gauss > (1 << 20)) throw KioError("the model has more than 2^20 components");
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<FgmmAccumulator> a(new FgmmAccumulator);
  a->impl_.reset(new FgmmAccumulator::Impl);
  FgmmAccumulator::Impl& I = *a->impl_;
  I.device = device;
  I.num_gauss = num_gauss;
  I.dim = dim;
  I.flags = AugmentGmmFlags(flags);
  I.occ.Alloc((size_t)num_gauss * 8);
  I.mean.Alloc((size_t)num_gauss * dim * 8);
  I.cov.Alloc((size_t)num_gauss * Tri(dim) * 8);
  Check(hipMemset(I.occ.p, 0, I.occ.cap), "hipMemset");
  Check(hipMemset(I.mean.p, 0, I.mean.cap), "hipMemset");
  Check(hipMemset(I.cov.p, 0, I.cov.cap), "hipMemset");
  return a.release();
}

namespace {

// the work items, then the accumulation.  a: everything but item_start, num_items, partial and the accumulators.  Returns the ms.
float RunAcc(FgmmAccumulator::Impl& I, FgmmAccArgs a, bool timed) {
  I.item_start.Reserve((size_t)(I.num_gauss + 1) * 4);
  a.dim = I.dim;
  a.num_gauss = I.num_gauss;
  a.flags = I.flags;
  a.item_start = I.item_start.as<int32_t>();
  a.occ = I.occ.as<double>();
  a.mean = I.mean.as<double>();
  a.cov = I.cov.as<double>();
  // the grid and the partial sums are sized by a bound on the number of items, so that no count comes back between the launches:
  // a bucket that is not empty has at most one chunk that is not full
  const int64_t bound = a.pairs / kFgmmAccPairChunk + std::min<int64_t>(I.num_gauss, a.pairs);
  const size_t partial_bytes = (size_t)bound * (1 + I.dim + Tri(I.dim)) * 8;
  if (bound >= INT32_MAX || partial_bytes > ((size_t)8 << 30))
    throw KioError("fgmm accumulate: " + std::to_string(a.pairs) + " pairs on " + std::to_string(I.num_gauss) + " Gaussians of dimension " +
                   std::to_string(I.dim) + " need " + std::to_string(partial_bytes >> 20) + " MiB of partial sums; the limit of one call is 8192 MiB");
  a.num_items = (int)bound;
  I.partial.Reserve(partial_bytes);
  a.partial = I.partial.as<double>();
  EventTimer tm(timed);
  tm.Start();
  Check(launch_fgmm_acc_items(a, nullptr), "fgmm_acc_items launch");
  Check(launch_fgmm_acc(a, nullptr), "fgmm_acc launch");
  return timed ? tm.Stop() : 0.f;
}

}  // namespace

void FgmmAccAdd(FgmmAccumulator* acc, const float* feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w,
                float* device_ms2) {
  if (device_ms2) device_ms2[0] = device_ms2[1] = 0.f;
  FgmmAccumulator::Impl& I = *acc->impl_;
  if (rows < 0 || rows > INT32_MAX - 1 || !post_off) throw KioError("fgmm accumulate: bad argument");
  if (post_off[0] != 0) throw KioError("fgmm accumulate: the posterior offsets must start at 0");
  for (int64_t t = 0; t < rows; ++t)
    if (post_off[t + 1] < post_off[t]) throw KioError("fgmm accumulate: the posterior offsets must not decrease");
  const int64_t pairs = post_off[rows];
  if (pairs == 0) return;
  if (!feats || !post_idx || !post_w) throw KioError("fgmm accumulate: null buffer");
  for (int64_t i = 0; i < pairs; ++i)
    if (post_idx[i] < 0 || post_idx[i] >= I.num_gauss)
      throw KioError("fgmm accumulate: the posteriors name Gaussian " + std::to_string(post_idx[i]) + "; the accumulators have " + std::to_string(I.num_gauss));
  std::vector<int32_t> frame((size_t)pairs);
  for (int64_t t = 0; t < rows; ++t)
    for (int32_t i = post_off[t]; i < post_off[t + 1]; ++i) frame[i] = (int32_t)t;
  UseDevice(I.device, kWhoNeeds);
  I.feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  I.idx.Upload(post_idx, (size_t)pairs * 4, "copy the posterior indices");
  I.w.Upload(post_w, (size_t)pairs * 4, "copy the posteriors");
  I.frame.Upload(frame, "copy the posteriors' frames");
  // the counting sort of ubm_kernels.h, on pairs of one slot each
  UbmFullArgs s;
  memset(&s, 0, sizeof s);
  s.rows = pairs;
  s.n = 1;
  s.dim = I.dim;
  s.num_gauss = I.num_gauss;
  s.num_chunks = (int)((pairs + kUbmSortChunk - 1) / kUbmSortChunk);
  const size_t hist_bytes = (size_t)I.num_gauss * s.num_chunks * 4;
  I.rank.Reserve((size_t)pairs * 4);
  I.hist.Reserve(hist_bytes);
  I.start.Reserve((size_t)(I.num_gauss + 1) * 4);
  I.sorted.Reserve((size_t)pairs * 4);
  Check(hipMemsetAsync(I.hist.p, 0, hist_bytes, nullptr), "hipMemsetAsync");
  s.gselect = I.idx.as<int32_t>();
  s.local_rank = I.rank.as<int32_t>();
  s.chunk_hist = I.hist.as<int32_t>();
  s.bucket_start = I.start.as<int32_t>();
  s.sorted = I.sorted.as<int32_t>();
  EventTimer tm(device_ms2 != nullptr);
  tm.Start();
  Check(launch_ubm_bucket_sort(s, nullptr), "ubm_bucket_sort launch");
  if (device_ms2) device_ms2[0] = tm.Stop();
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = I.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = I.frame.as<int32_t>();
  a.n = 1;
  a.pair_w = I.w.as<float>();
  a.sorted = I.sorted.as<int32_t>();
  a.bucket_start = I.start.as<int32_t>();
  const float ms = RunAcc(I, a, device_ms2 != nullptr);
  if (device_ms2) device_ms2[1] = ms;
  Check(hipDeviceSynchronize(), "fgmm_acc");
}

void FgmmAccAddGselect(FgmmAccumulator* acc, const UbmModel& full, const float* feats, int64_t rows, const int32_t* gselect, int n, float* logsum,
                       float* device_ms4) {
  if (device_ms4) device_ms4[0] = device_ms4[1] = device_ms4[2] = device_ms4[3] = 0.f;
  FgmmAccumulator::Impl& I = *acc->impl_;
  if (rows < 0) throw KioError("fgmm accumulate: bad argument");
  if (full.full() && (full.num_gauss() != I.num_gauss || full.dim() != I.dim))
    throw KioError("fgmm accumulate: the model has " + std::to_string(full.num_gauss()) + " components of dimension " + std::to_string(full.dim()) +
                   ", the accumulators " + std::to_string(I.num_gauss) + " of dimension " + std::to_string(I.dim));
  if (full.device() != I.device) throw KioError("fgmm accumulate: the model and the accumulators are on different devices");
  CheckUbmSelection("fgmm accumulate", full, gselect, rows, n);
  if (rows == 0) return;
  if (!feats || !logsum) throw KioError("fgmm accumulate: null buffer");
  if (rows * n >= INT32_MAX) throw KioError("fgmm accumulate: more than 2^31 pairs in one call");
  UseDevice(I.device, kWhoNeeds);
  I.post.Run(full, feats, gselect, rows, n, 0.f, true, device_ms4);
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = I.post.feats.as<float>();
  a.rows = rows;
  a.pairs = rows * n;
  a.pair_frame = nullptr;
  a.n = n;
  a.pair_w = I.post.slot_post.as<float>();
  a.sorted = I.post.sorted.as<int32_t>();
  a.bucket_start = I.post.start.as<int32_t>();
  const float ms = RunAcc(I, a, device_ms4 != nullptr);
  if (device_ms4) device_ms4[3] = ms;
  I.post.logsum.Download(logsum, (size_t)rows * 4, "copy the log-sums");
}

void FgmmAccGet(const FgmmAccumulator& acc, double* occ, double* mean, double* cov) {
  const FgmmAccumulator::Impl& I = *acc.impl_;
  UseDevice(I.device, kWhoNeeds);
  if (occ) I.occ.Download(occ, (size_t)I.num_gauss * 8, "copy the occupancies");
  if (mean) I.mean.Download(mean, (size_t)I.num_gauss * I.dim * 8, "copy the mean accumulators");
  if (cov) I.cov.Download(cov, (size_t)I.num_gauss * Tri(I.dim) * 8, "copy the covariance accumulators");
}

}  // namespace xv
