#include "dubm_train.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <sstream>

#include "device.h"
#include "dubm_train_kernels.h"
#include "ivex_train.h"
#include "ubm_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "diagonal UBM training needs";

std::string FlagLetters(int flags) {
  std::string s;
  if (flags & kFgmmFlagMeans) s += 'm';
  if (flags & kFgmmFlagVariances) s += 'v';
  if (flags & kFgmmFlagWeights) s += 'w';
  return s;
}

}  // namespace

uint64_t DgmmDrawA(uint64_t seed, uint64_t e) { return Mix53(seed, 2 * e); }
uint64_t DgmmDrawB(uint64_t seed, uint64_t e) { return Mix53(seed, 2 * e + 1); }
double DgmmGauss(uint64_t seed, uint64_t e) {
  const double two_pi = 6.283185307179586476925286766559;
  const double u1 = ((double)DgmmDrawA(seed, e) + 1.0) / 9007199254740992.0, u2 = (double)DgmmDrawB(seed, e) / 9007199254740992.0;
  return sqrt(-2.0 * log(u1)) * cos(two_pi * u2);
}

void DgmmAccs::Init(int g, int d, int f) {
  if (g < 1 || d < 1 || f < 0 || f > 7) throw KioError("GMM accumulators: bad shape or flags");
  num_gauss = g;
  dim = d;
  flags = AugmentGmmFlags(f);
  occ.assign((size_t)g, 0.0);
  mean.assign((size_t)g * d, 0.0);
  var.assign((size_t)g * d, 0.0);
}

void ReadDgmmAccsFile(const std::string& rxfilename, bool add, DgmmAccs* a) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
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
    ExpectToken(in, binary, "<DIAGVARACCS>");
    ReadMatrix(in, binary, &m);
    if (m.rows != G || m.cols != dim) throw KioError("<DIAGVARACCS> is " + std::to_string(m.rows) + " x " + std::to_string(m.cols));
    for (size_t i = 0; i < (size_t)G * dim; ++i) a->var[i] += (double)m.Data()[i];
  }
  ExpectToken(in, binary, "</GMMACCS>");
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
}

void WriteDgmmAccsFile(const std::string& wxfilename, bool binary, const DgmmAccs& a) {
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
    m.data.assign(a.var.begin(), a.var.end());
    WriteToken(out, binary, "<DIAGVARACCS>");
    WriteMatrix(out, binary, m);
  }
  WriteToken(out, binary, "</GMMACCS>");
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
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
    for (size_t i = 0; i < G * D; ++i) q += a.var[i] * (double)m.inv_vars[i];
    obj -= 0.5 * q;
  }
  return obj;
}

}  // namespace

void DgmmEst(const DgmmAccs& accs, int update_flags, const DgmmEstOptions& o, DiagGmmData* model, DgmmEstResult* res) {
  const int G = model->num_gauss, D = model->dim;
  if (accs.num_gauss != G || accs.dim != D)
    throw KioError("the accumulators (" + std::to_string(accs.num_gauss) + " components of dimension " + std::to_string(accs.dim) + ") are not the model's (" +
                   std::to_string(G) + " of dimension " + std::to_string(D) + ")");
  if (update_flags & ~accs.flags)
    throw KioError("the update flags '" + FlagLetters(update_flags) + "' name statistics that the accumulators (flags '" + FlagLetters(accs.flags) + "') do not have");
  *res = DgmmEstResult();
  const bool upd_m = update_flags & kFgmmFlagMeans, upd_v = update_flags & kFgmmFlagVariances, upd_w = update_flags & kFgmmFlagWeights;
  const bool has_m = accs.flags & kFgmmFlagMeans, has_v = accs.flags & kFgmmFlagVariances;
  ComputeGconsts(model);
  res->objf_before = MlObjective(accs, *model);
  double occ_sum = 0.0;
  for (int g = 0; g < G; ++g) occ_sum += accs.occ[g];
  res->count = occ_sum;
  std::vector<double> w((size_t)G), mu((size_t)D), var((size_t)D);
  std::vector<char> remove((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    const double occ = accs.occ[g];
    const double prob = occ_sum > 0.0 ? occ / occ_sum : 1.0 / G;
    float* iv = model->inv_vars.data() + (size_t)g * D;
    float* mi = model->means_invvars.data() + (size_t)g * D;
    if (occ > o.min_gaussian_occupancy && prob > o.min_gaussian_weight) {
      w[g] = prob;
      if (!has_m) continue;
      int floored = 0;
      for (int d = 0; d < D; ++d) {
        const double mu_old = (double)mi[d] / (double)iv[d];
        mu[d] = accs.mean[(size_t)g * D + d] / occ;
        if (has_v) {
          double v = accs.var[(size_t)g * D + d] / occ - mu[d] * mu[d];
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
      if (!upd_m && !upd_v) continue;
      for (int d = 0; d < D; ++d) {
        const double inv = upd_v ? 1.0 / var[d] : (double)iv[d];
        if (upd_v) iv[d] = (float)inv;
        mi[d] = (float)(mu[d] * inv);
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
    DiagGmmData out;
    out.dim = D;
    double sum = 0.0;
    for (int g = 0; g < G; ++g)
      if (!remove[g]) sum += (double)model->weights[g];
    for (int g = 0; g < G; ++g) {
      if (remove[g]) continue;
      ++out.num_gauss;
      out.weights.push_back((float)((double)model->weights[g] / sum));
      out.means_invvars.insert(out.means_invvars.end(), model->means_invvars.begin() + (size_t)g * D, model->means_invvars.begin() + (size_t)(g + 1) * D);
      out.inv_vars.insert(out.inv_vars.end(), model->inv_vars.begin() + (size_t)g * D, model->inv_vars.begin() + (size_t)(g + 1) * D);
    }
    ComputeGconsts(&out);
    *model = out;
  }
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
  int device = 0, num_gauss = 0, dim = 0, flags = 0;
  DevBuf occ, mean, var;                                        // the running accumulators
  DevBuf feats, idx, w, frame, gselect;                         // a call's inputs
  DevBuf rank, hist, start, sorted;                             // the sort
  DevBuf ll, count, pidx, post, logsum, slot_post;              // the sparse E-step
  DevBuf item_start, partial, dense_post;
  DevBuf resident;                                              // DgmmAccSetFrames
  int64_t resident_rows = 0;

  void Zero() {
    Check(hipMemset(occ.p, 0, (size_t)num_gauss * 8), "hipMemset");
    Check(hipMemset(mean.p, 0, (size_t)num_gauss * dim * 8), "hipMemset");
    Check(hipMemset(var.p, 0, (size_t)num_gauss * dim * 8), "hipMemset");
  }
};

DgmmAccumulator::~DgmmAccumulator() {}
int DgmmAccumulator::num_gauss() const { return impl_->num_gauss; }
int DgmmAccumulator::dim() const { return impl_->dim; }
int DgmmAccumulator::flags() const { return impl_->flags; }

DgmmAccumulator* DgmmAccCreate(int device, int num_gauss, int dim, int flags) {
  if (num_gauss < 1 || dim < 1 || flags < 0 || flags > 7) throw KioError("dgmm accumulator: bad argument");
  if (dim > kDgmmMaxDim)
    throw KioError("the dimension " + std::to_string(dim) + " is above the accumulation kernels' limit of " + std::to_string(kDgmmMaxDim));
  if (num_gauss > (1 << 20)) throw KioError("the model has more than 2^20 components");
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<DgmmAccumulator> a(new DgmmAccumulator);
  a->impl_.reset(new DgmmAccumulator::Impl);
  DgmmAccumulator::Impl& I = *a->impl_;
  I.device = device;
  I.dim = dim;
  I.flags = AugmentGmmFlags(flags);
  DgmmAccReset(a.get(), num_gauss);
  return a.release();
}

void DgmmAccReset(DgmmAccumulator* acc, int num_gauss) {
  DgmmAccumulator::Impl& I = *acc->impl_;
  if (num_gauss < 1 || num_gauss > (1 << 20)) throw KioError("dgmm accumulator: bad number of components");
  UseDevice(I.device, kWhoNeeds);
  I.num_gauss = num_gauss;
  I.occ.Reserve((size_t)num_gauss * 8);
  I.mean.Reserve((size_t)num_gauss * I.dim * 8);
  I.var.Reserve((size_t)num_gauss * I.dim * 8);
  I.Zero();
}

namespace {

using Impl = DgmmAccumulator::Impl;

// the counting sort of ubm_kernels.h on `pairs` pairs whose Gaussians are d_gauss; returns the ms when timed
float SortPairs(Impl& I, const int32_t* d_gauss, int64_t pairs, bool timed) {
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
  s.gselect = d_gauss;
  s.local_rank = I.rank.as<int32_t>();
  s.chunk_hist = I.hist.as<int32_t>();
  s.bucket_start = I.start.as<int32_t>();
  s.sorted = I.sorted.as<int32_t>();
  EventTimer tm(timed);
  tm.Start();
  Check(launch_ubm_bucket_sort(s, nullptr), "ubm_bucket_sort launch");
  return timed ? tm.Stop() : 0.f;
}

// the work items, the partial sums and the reduction.  a: feats, rows, pairs, pair_frame / n, pair_w.
float RunSparseAcc(Impl& I, FgmmAccArgs a, bool timed) {
  I.item_start.Reserve((size_t)(I.num_gauss + 1) * 4);
  a.dim = I.dim;
  a.num_gauss = I.num_gauss;
  a.flags = I.flags;
  a.sorted = I.sorted.as<int32_t>();
  a.bucket_start = I.start.as<int32_t>();
  a.item_start = I.item_start.as<int32_t>();
  a.occ = I.occ.as<double>();
  a.mean = I.mean.as<double>();
  a.cov = I.var.as<double>();
  // a bucket that is not empty has at most one chunk that is not full: a bound that needs no count from the device
  const int64_t bound = a.pairs / kFgmmAccPairChunk + std::min<int64_t>(I.num_gauss, a.pairs);
  const size_t partial_bytes = (size_t)bound * (1 + 2 * I.dim) * 8;
  if (bound >= INT32_MAX) throw KioError("dgmm accumulate: too many pairs in one call");
  a.num_items = (int)bound;
  I.partial.Reserve(partial_bytes);
  a.partial = I.partial.as<double>();
  EventTimer tm(timed);
  tm.Start();
  Check(launch_fgmm_acc_items(a, nullptr), "fgmm_acc_items launch");
  Check(launch_dgmm_acc(a, nullptr), "dgmm_acc launch");
  return timed ? tm.Stop() : 0.f;
}

DgmmModelArgs ModelArgs(const Impl& I, const UbmModel& diag, const char* who) {
  const UbmDiagView v = UbmDiagArrays(diag);
  if (v.num_gauss != I.num_gauss || v.dim != I.dim)
    throw KioError(std::string(who) + ": the model has " + std::to_string(v.num_gauss) + " components of dimension " + std::to_string(v.dim) +
                   ", the accumulators " + std::to_string(I.num_gauss) + " of dimension " + std::to_string(I.dim));
  if (v.device != I.device) throw KioError(std::string(who) + ": the model and the accumulators are on different devices");
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
  const size_t partial_bytes = (size_t)I.num_gauss * a.num_chunks * (1 + 2 * I.dim) * 8;
  if (partial_bytes > ((size_t)8 << 30))
    throw KioError("dgmm dense accumulate: " + std::to_string(a.rows) + " frames on " + std::to_string(I.num_gauss) + " Gaussians of dimension " +
                   std::to_string(I.dim) + " need " + std::to_string(partial_bytes >> 20) + " MiB of partial sums; the limit of one call is 8192 MiB");
  I.partial.Reserve(partial_bytes);
  a.partial = I.partial.as<double>();
  const bool timed = ms_acc != nullptr;
  EventTimer tm(timed, 3);
  tm.Mark();
  Check(launch_dgmm_dense_acc(a, nullptr), "dgmm_dense_acc launch");
  tm.Mark();
  DgmmReduceArgs r;
  memset(&r, 0, sizeof r);
  r.dim = I.dim;
  r.num_gauss = I.num_gauss;
  r.flags = I.flags;
  r.num_chunks = a.num_chunks;
  r.partial = a.partial;
  r.occ = I.occ.as<double>();
  r.mean = I.mean.as<double>();
  r.var = I.var.as<double>();
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
  Impl& I = *acc->impl_;
  if (rows < 0 || rows > INT32_MAX - 1 || !post_off) throw KioError("dgmm accumulate: bad argument");
  if (post_off[0] != 0) throw KioError("dgmm accumulate: the posterior offsets must start at 0");
  for (int64_t t = 0; t < rows; ++t)
    if (post_off[t + 1] < post_off[t]) throw KioError("dgmm accumulate: the posterior offsets must not decrease");
  const int64_t pairs = post_off[rows];
  if (pairs == 0) return;
  if (!feats || !post_idx || !post_w) throw KioError("dgmm accumulate: null buffer");
  for (int64_t i = 0; i < pairs; ++i)
    if (post_idx[i] < 0 || post_idx[i] >= I.num_gauss)
      throw KioError("dgmm accumulate: the posteriors name Gaussian " + std::to_string(post_idx[i]) + "; the accumulators have " + std::to_string(I.num_gauss));
  std::vector<int32_t> frame((size_t)pairs);
  for (int64_t t = 0; t < rows; ++t)
    for (int32_t i = post_off[t]; i < post_off[t + 1]; ++i) frame[i] = (int32_t)t;
  UseDevice(I.device, kWhoNeeds);
  I.feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  I.idx.Upload(post_idx, (size_t)pairs * 4, "copy the posterior indices");
  I.w.Upload(post_w, (size_t)pairs * 4, "copy the posteriors");
  I.frame.Upload(frame, "copy the posteriors' frames");
  const float ms_sort = SortPairs(I, I.idx.as<int32_t>(), pairs, device_ms2 != nullptr);
  FgmmAccArgs a;
  memset(&a, 0, sizeof a);
  a.feats = I.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = I.frame.as<int32_t>();
  a.n = 1;
  a.pair_w = I.w.as<float>();
  const float ms = RunSparseAcc(I, a, device_ms2 != nullptr);
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
    if (gselect[i] < 0 || gselect[i] >= I.num_gauss)
      throw KioError("dgmm accumulate: the selection names Gaussian " + std::to_string(gselect[i]) + "; the model has " + std::to_string(I.num_gauss));
  UseDevice(I.device, kWhoNeeds);
  const bool timed = device_ms4 != nullptr;
  I.feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  I.gselect.Upload(gselect, (size_t)pairs * 4, "copy the selection");
  I.ll.Reserve((size_t)pairs * 4);
  I.count.Reserve((size_t)rows * 4);
  I.pidx.Reserve((size_t)pairs * 4);
  I.post.Reserve((size_t)pairs * 4);
  I.slot_post.Reserve((size_t)pairs * 4);
  I.logsum.Reserve((size_t)rows * 4);
  // the pairs (frame, slot) are bucketed by their Gaussian: n = 1 over rows * n pairs is the same sort as n over rows frames
  const float ms_sort = SortPairs(I, I.gselect.as<int32_t>(), pairs, timed);
  sel.feats = I.feats.as<float>();
  sel.rows = rows;
  sel.n = n;
  sel.gselect = I.gselect.as<int32_t>();
  sel.ll = I.ll.as<float>();
  UbmFullArgs p;
  memset(&p, 0, sizeof p);
  p.rows = rows;
  p.dim = I.dim;
  p.num_gauss = I.num_gauss;
  p.n = n;
  p.gselect = I.gselect.as<int32_t>();
  p.bucket_start = I.start.as<int32_t>();
  p.sorted = I.sorted.as<int32_t>();
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
  a.feats = I.feats.as<float>();
  a.rows = rows;
  a.pairs = pairs;
  a.pair_frame = nullptr;
  a.n = n;
  a.pair_w = I.slot_post.as<float>();
  const float ms = RunSparseAcc(I, a, timed);
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
  UseDevice(I.device, kWhoNeeds);
  I.feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  I.dense_post.Upload(post, (size_t)rows * I.num_gauss * 4, "copy the posteriors");
  DgmmDenseArgs a;
  memset(&a, 0, sizeof a);
  a.model.dim = I.dim;
  a.model.num_gauss = I.num_gauss;
  a.feats = I.feats.as<float>();
  a.rows = rows;
  a.post = I.dense_post.as<float>();
  RunDense(I, a, nullptr, nullptr);
  Check(hipDeviceSynchronize(), "dgmm_dense_acc");
}

void DgmmAccSetFrames(DgmmAccumulator* acc, const float* feats, int64_t rows) {
  Impl& I = *acc->impl_;
  if (rows < 1 || !feats) throw KioError("dgmm dense accumulate: no frames");
  UseDevice(I.device, kWhoNeeds);
  I.resident.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
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
  UseDevice(I.device, kWhoNeeds);
  if (feats) I.feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  I.logsum.Reserve((size_t)rows * 4);
  a.feats = feats ? I.feats.as<float>() : I.resident.as<float>();
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
  const Impl& I = *acc.impl_;
  UseDevice(I.device, kWhoNeeds);
  if (occ) I.occ.Download(occ, (size_t)I.num_gauss * 8, "copy the occupancies");
  if (mean) I.mean.Download(mean, (size_t)I.num_gauss * I.dim * 8, "copy the mean accumulators");
  if (var) I.var.Download(var, (size_t)I.num_gauss * I.dim * 8, "copy the variance accumulators");
}

}  // namespace xv
