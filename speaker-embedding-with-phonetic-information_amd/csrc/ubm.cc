#include "ubm.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>

#include "device.h"
#include "ubm_kernels.h"

// DeltaScales is compared with tests/ubm_ref.py for equality: float(j) * scale and the sum are two roundings, not a fused one
#pragma clang fp contract(off)

namespace xv {
namespace {

const char kWhoNeeds[] = "the UBM kernels need";

// Cholesky factor of the packed lower triangle `p` (as doubles): l [dim][dim] lower; false: not positive definite
bool Cholesky(const float* p, int dim, std::vector<double>* l) {
  l->assign((size_t)dim * dim, 0.0);
  double* L = l->data();
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = (double)p[(size_t)i * (i + 1) / 2 + j];
      for (int k = 0; k < j; ++k) s -= L[i * dim + k] * L[j * dim + k];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[i * dim + i] = sqrt(s);
      } else {
        L[i * dim + j] = s / L[j * dim + j];
      }
    }
  return true;
}

// the inverse of a lower-triangular matrix, in place of *inv
void InvertLower(const std::vector<double>& l, int dim, std::vector<double>* inv) {
  inv->assign((size_t)dim * dim, 0.0);
  for (int c = 0; c < dim; ++c) {
    (*inv)[c * dim + c] = 1.0 / l[c * dim + c];
    for (int i = c + 1; i < dim; ++i) {
      double s = 0.0;
      for (int k = c; k < i; ++k) s -= l[i * dim + k] * (*inv)[k * dim + c];
      (*inv)[i * dim + c] = s / l[i * dim + i];
    }
  }
}

const double kLog2Pi = 1.8378770664093454835606594728112;

}  // namespace

void DeltaScales(int order, int window, std::vector<std::vector<float>>* scales) {
  if (order < 0 || order > kDeltaMaxOrder) throw KioError("delta-order must be between 0 and " + std::to_string(kDeltaMaxOrder));
  if (window < 1 || window > 1000) throw KioError("delta-window must be between 1 and 1000");
  scales->assign((size_t)order + 1, std::vector<float>());
  (*scales)[0].assign(1, 1.0f);
  for (int i = 1; i <= order; ++i) {
    const std::vector<float>& prev = (*scales)[i - 1];
    std::vector<float>& cur = (*scales)[i];
    cur.assign(prev.size() + 2 * (size_t)window, 0.0f);
    float normalizer = 0.0f;
    for (int j = -window; j <= window; ++j) {
      normalizer += (float)(j * j);
      for (size_t k = 0; k < prev.size(); ++k) {
        const float prod = (float)j * prev[k];
        cur[k + j + window] = cur[k + j + window] + prod;
      }
    }
    const float alpha = (float)(1.0 / (double)normalizer);
    for (float& v : cur) v = v * alpha;
  }
}

void AddDeltas(int device, const float* feats, const int32_t* row_off, int n, int cols, int order, int window, int truncate, float* out,
               float* device_ms) {
  if (device_ms) *device_ms = 0.f;
  const int64_t rows = CheckOffsets("add-deltas", row_off, n);
  if (cols < 1 || truncate < 0) throw KioError("add-deltas: bad argument");
  if (truncate > cols) throw KioError("Cannot truncate features as dimension " + std::to_string(cols) + " is smaller than truncation dimension " + std::to_string(truncate));
  std::vector<std::vector<float>> scales;
  DeltaScales(order, window, &scales);
  if (rows == 0) return;
  if (!feats || !out) throw KioError("add-deltas: null buffer");
  const int dim = truncate > 0 ? truncate : cols;
  UseDevice(device, kWhoNeeds);
  DeltaArgs a;
  memset(&a, 0, sizeof a);
  std::vector<float> flat;
  for (int i = 0; i <= order; ++i) {
    a.scale_off[i] = (int)flat.size();
    flat.insert(flat.end(), scales[i].begin(), scales[i].end());
  }
  WorkItems items;
  for (int u = 0; u < n; ++u) items.Add(u, CeilDiv(row_off[u + 1] - row_off[u], kDeltaRowBlock));
  DevBuf d_feats, d_off, d_scales, d_out;
  d_feats.Upload(feats, (size_t)rows * cols * 4, "copy features");
  d_off.Upload(row_off, (size_t)(n + 1) * 4, "copy row offsets");
  d_scales.Upload(flat, "copy delta scales");
  items.Upload();
  const size_t out_bytes = (size_t)rows * (order + 1) * dim * 4;
  d_out.Alloc(out_bytes);
  a.feats = d_feats.as<float>();
  a.in_stride = cols;
  a.dim = dim;
  a.row_off = d_off.as<int32_t>();
  a.n = n;
  a.order = order;
  a.window = window;
  a.scales = d_scales.as<float>();
  a.item_mat = items.d_unit.as<int32_t>();
  a.item_blk = items.d_blk.as<int32_t>();
  a.n_items = items.size();
  a.out = d_out.as<float>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_add_deltas(a, nullptr), "add_deltas launch");
  if (device_ms) *device_ms = tm.Stop();
  d_out.Download(out, out_bytes, "copy delta features");
}

// ---------------------------------------------------------------------------------------------------------------------------------
int ComputeGconsts(DiagGmmData* m) {
  const int G = m->num_gauss, D = m->dim;
  m->gconsts.assign((size_t)G, 0.f);
  int bad = 0;
  for (int g = 0; g < G; ++g) {
    double gc = log((double)m->weights[g]) - 0.5 * kLog2Pi * D;
    for (int d = 0; d < D; ++d) {
      const double iv = m->inv_vars[(size_t)g * D + d], mi = m->means_invvars[(size_t)g * D + d];
      gc += 0.5 * log(iv) - 0.5 * mi * mi / iv;
    }
    if (!std::isfinite(gc)) {
      gc = -std::numeric_limits<double>::infinity();
      ++bad;
    }
    m->gconsts[g] = (float)gc;
  }
  return bad;
}

int ComputeGconsts(FullGmmData* m) {
  const int G = m->num_gauss, D = m->dim;
  const size_t tri = (size_t)D * (D + 1) / 2;
  m->gconsts.assign((size_t)G, 0.f);
  int bad = 0;
  std::vector<double> l, linv, y((size_t)D);
  for (int g = 0; g < G; ++g) {
    double gc = -std::numeric_limits<double>::infinity();
    if (Cholesky(m->inv_covars.data() + (size_t)g * tri, D, &l)) {
      // Sigma^-1 = L L': log det Sigma = -2 sum log L_ii;  b' Sigma b = |L^-1 b|^2
      double logdet_inv = 0.0, quad = 0.0;
      for (int i = 0; i < D; ++i) {
        logdet_inv += 2.0 * log(l[(size_t)i * D + i]);
        double s = (double)m->means_invcovars[(size_t)g * D + i];
        for (int k = 0; k < i; ++k) s -= l[(size_t)i * D + k] * y[k];
        y[i] = s / l[(size_t)i * D + i];
        quad += y[i] * y[i];
      }
      gc = log((double)m->weights[g]) - 0.5 * kLog2Pi * D - 0.5 * (-logdet_inv + quad);
    }
    if (!std::isfinite(gc)) {
      gc = -std::numeric_limits<double>::infinity();
      ++bad;
    }
    m->gconsts[g] = (float)gc;
  }
  return bad;
}

void FullGmmToDiag(const FullGmmData& full, DiagGmmData* diag) {
  const int G = full.num_gauss, D = full.dim;
  const size_t tri = (size_t)D * (D + 1) / 2;
  *diag = DiagGmmData();
  diag->num_gauss = G;
  diag->dim = D;
  diag->weights = full.weights;
  diag->means_invvars.assign((size_t)G * D, 0.f);
  diag->inv_vars.assign((size_t)G * D, 0.f);
  std::vector<double> l, linv, sigma((size_t)D * D);
  for (int g = 0; g < G; ++g) {
    if (!Cholesky(full.inv_covars.data() + (size_t)g * tri, D, &l))
      throw KioError("the inverse covariance of component " + std::to_string(g) + " is not positive definite: it cannot be inverted");
    InvertLower(l, D, &linv);
    for (int i = 0; i < D; ++i)   // Sigma = L^-T L^-1
      for (int j = 0; j <= i; ++j) {
        double s = 0.0;
        for (int k = i; k < D; ++k) s += linv[(size_t)k * D + i] * linv[(size_t)k * D + j];
        sigma[(size_t)i * D + j] = sigma[(size_t)j * D + i] = s;
      }
    for (int i = 0; i < D; ++i) {
      double mean = 0.0;
      for (int j = 0; j < D; ++j) mean += sigma[(size_t)i * D + j] * (double)full.means_invcovars[(size_t)g * D + j];
      const double iv = 1.0 / sigma[(size_t)i * D + i];
      diag->inv_vars[(size_t)g * D + i] = (float)iv;
      diag->means_invvars[(size_t)g * D + i] = (float)(mean * iv);
    }
  }
  ComputeGconsts(diag);
}

void ReadDiagGmmFile(const std::string& rxfilename, DiagGmmData* m) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ReadDiagGmm(in, binary, m);
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
  ComputeGconsts(m);
}

void ReadFullGmmFile(const std::string& rxfilename, FullGmmData* m) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ReadFullGmm(in, binary, m);
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
  ComputeGconsts(m);
}

void WriteDiagGmmFile(const std::string& wxfilename, bool binary, const DiagGmmData& m) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteDiagGmm(out, binary, m);
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

void WriteFullGmmFile(const std::string& wxfilename, bool binary, const FullGmmData& m) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteFullGmm(out, binary, m);
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct UbmModel::Impl {
  int device = 0, num_gauss = 0, dim = 0, gauss_pad = 0;
  bool full = false;
  DevBuf gconst, a, b;   // diagonal: m_t, v_t;  full: lin, inv_covars
};

UbmModel::~UbmModel() {}
int UbmModel::device() const { return impl_->device; }
int UbmModel::num_gauss() const { return impl_->num_gauss; }
int UbmModel::dim() const { return impl_->dim; }
bool UbmModel::full() const { return impl_->full; }

namespace {

void CheckModelShape(int num_gauss, int dim, const void* p0, const void* p1, const void* p2) {
  if (num_gauss < 1 || dim < 1 || !p0 || !p1 || !p2) throw KioError("ubm model: bad argument");
  if (dim > kUbmMaxDim)
    throw KioError("the model's dimension " + std::to_string(dim) + " is above the device kernels' limit of " + std::to_string(kUbmMaxDim));
  if (num_gauss > (1 << 20)) throw KioError("the model has more than 2^20 components");
}

}  // namespace

UbmModel* UbmDiagCreate(int device, int num_gauss, int dim, const float* gconsts, const float* means_invvars, const float* inv_vars) {
  CheckModelShape(num_gauss, dim, gconsts, means_invvars, inv_vars);
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<UbmModel> m(new UbmModel);
  m->impl_.reset(new UbmModel::Impl);
  UbmModel::Impl& I = *m->impl_;
  I.device = device;
  I.num_gauss = num_gauss;
  I.dim = dim;
  I.gauss_pad = (num_gauss + kUbmGaussTile - 1) / kUbmGaussTile * kUbmGaussTile;
  // transposed, so that the threads of a tile read consecutive addresses; -1/2 folded into the inverse variances (exact)
  std::vector<float> gc((size_t)I.gauss_pad, 0.f), mt((size_t)dim * I.gauss_pad, 0.f), vt((size_t)dim * I.gauss_pad, 0.f);
  for (int g = 0; g < num_gauss; ++g) {
    gc[g] = gconsts[g];
    for (int d = 0; d < dim; ++d) {
      mt[(size_t)d * I.gauss_pad + g] = means_invvars[(size_t)g * dim + d];
      vt[(size_t)d * I.gauss_pad + g] = -0.5f * inv_vars[(size_t)g * dim + d];
    }
  }
  I.gconst.Upload(gc, "copy gconsts");
  I.a.Upload(mt, "copy the diagonal model");
  I.b.Upload(vt, "copy the diagonal model");
  return m.release();
}

UbmModel* UbmFullCreate(int device, int num_gauss, int dim, const float* gconsts, const float* means_invcovars, const float* inv_covars) {
  CheckModelShape(num_gauss, dim, gconsts, means_invcovars, inv_covars);
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<UbmModel> m(new UbmModel);
  m->impl_.reset(new UbmModel::Impl);
  UbmModel::Impl& I = *m->impl_;
  I.device = device;
  I.num_gauss = num_gauss;
  I.dim = dim;
  I.full = true;
  I.gconst.Upload(gconsts, (size_t)num_gauss * 4, "copy gconsts");
  I.a.Upload(means_invcovars, (size_t)num_gauss * dim * 4, "copy the full model");
  I.b.Upload(inv_covars, (size_t)num_gauss * ((size_t)dim * (dim + 1) / 2) * 4, "copy the full model");
  return m.release();
}

UbmDiagView UbmDiagArrays(const UbmModel& diag) {
  const UbmModel::Impl& I = *diag.impl_;
  if (I.full) throw KioError("the model is a full-covariance one; a diagonal model is needed here");
  return UbmDiagView{I.device, I.num_gauss, I.dim, I.gauss_pad, I.a.as<float>(), I.b.as<float>(), I.gconst.as<float>()};
}

void UbmGselect(const UbmModel& diag, const float* feats, const int32_t* row_off, int n_utts, int n, int32_t* idx, float* ll, float* device_ms) {
  if (device_ms) *device_ms = 0.f;
  const UbmModel::Impl& I = *diag.impl_;
  if (I.full) throw KioError("gselect: the model is a full-covariance one; Gaussian selection takes a diagonal model");
  const int64_t rows = CheckOffsets("gselect", row_off, n_utts);
  if (n < 1) throw KioError("gselect: n must be at least 1");
  if (n > kUbmMaxSelect) throw KioError("gselect: n = " + std::to_string(n) + " is above the device kernel's limit of " + std::to_string(kUbmMaxSelect) + " selected Gaussians");
  if (n > I.num_gauss) throw KioError("gselect: n = " + std::to_string(n) + " is above the model's " + std::to_string(I.num_gauss) + " Gaussians");
  if (rows == 0) return;
  if (!feats || !idx) throw KioError("gselect: null buffer");
  UseDevice(I.device, kWhoNeeds);
  DevBuf d_feats, d_idx, d_ll;
  d_feats.Upload(feats, (size_t)rows * I.dim * 4, "copy features");
  d_idx.Alloc((size_t)rows * n * 4);
  if (ll) d_ll.Alloc((size_t)rows * n * 4);
  UbmDiagArgs a;
  memset(&a, 0, sizeof a);
  a.feats = d_feats.as<float>();
  a.rows = rows;
  a.dim = I.dim;
  a.num_gauss = I.num_gauss;
  a.gauss_pad = I.gauss_pad;
  a.m_t = I.a.as<float>();
  a.v_t = I.b.as<float>();
  a.gconst = I.gconst.as<float>();
  a.n = n;
  a.out_idx = d_idx.as<int32_t>();
  a.out_ll = ll ? d_ll.as<float>() : nullptr;
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_ubm_diag_gselect(a, nullptr), "ubm_diag_gselect launch");
  if (device_ms) *device_ms = tm.Stop();
  Check(hipMemcpy(idx, d_idx.p, (size_t)rows * n * 4, hipMemcpyDeviceToHost), "copy the selection");
  if (ll) Check(hipMemcpy(ll, d_ll.p, (size_t)rows * n * 4, hipMemcpyDeviceToHost), "copy the log-likelihoods");
}

void CheckUbmSelection(const char* who, const UbmModel& full, const int32_t* gselect, int64_t rows, int n) {
  const UbmModel::Impl& I = *full.impl_;
  if (!I.full) throw KioError(std::string(who) + ": the model is a diagonal one; the posteriors take a full-covariance model");
  if (n < 1 || n > kUbmMaxSelect)
    throw KioError(std::string(who) + ": " + std::to_string(n) + " selected Gaussians per frame; the device kernels take 1 to " + std::to_string(kUbmMaxSelect));
  if (rows == 0) return;
  if (!gselect) throw KioError(std::string(who) + ": null buffer");
  for (int64_t i = 0; i < rows * n; ++i)
    if (gselect[i] < 0 || gselect[i] >= I.num_gauss)
      throw KioError(std::string(who) + ": the selection names Gaussian " + std::to_string(gselect[i]) + "; the model has " + std::to_string(I.num_gauss));
}

void UbmPostDevice::Scores(const UbmModel& full, const float* host_feats, const int32_t* host_gselect, int64_t rows, int n, UbmFullArgs* out,
                           EventTimer* tm) {
  const UbmModel::Impl& I = *full.impl_;
  const size_t pairs = (size_t)rows * n;
  UbmFullArgs& a = *out;
  memset(&a, 0, sizeof a);
  ll.Reserve(pairs * 4);
  feats.Upload(host_feats, (size_t)rows * I.dim * 4, "copy features");
  gselect.Upload(host_gselect, pairs * 4, "copy the selection");
  a.feats = feats.as<float>();
  a.rows = rows;
  a.dim = I.dim;
  a.num_gauss = I.num_gauss;
  a.inv_covars = I.b.as<float>();
  a.lin = I.a.as<float>();
  a.gconst = I.gconst.as<float>();
  a.n = n;
  a.gselect = gselect.as<int32_t>();
  // enough workgroups per Gaussian that an average bucket is a few passes of each
  const int64_t per_gauss = (int64_t)pairs / I.num_gauss;
  a.split = (int)std::max<int64_t>(1, std::min<int64_t>(64, per_gauss / (4 * kUbmFullFrameTile)));
  a.ll = ll.as<float>();
  tm->Mark();
  const int32_t seg_off[2] = {0, (int32_t)pairs};
  Check(sort.Run(a.gselect, (int64_t)pairs, seg_off, 1, I.num_gauss, nullptr), "bucket_sort launch");
  a.bucket_start = sort.start.as<int32_t>();   // Run sizes them
  a.sorted = sort.sorted.as<int32_t>();
  tm->Mark();
  Check(launch_ubm_full_loglike(a, nullptr), "ubm_full_loglike launch");
  tm->Mark();
}

void UbmPostDevice::Run(const UbmModel& full, const float* host_feats, const int32_t* host_gselect, int64_t rows, int n, float min_post,
                        bool with_slot_post, float* device_ms3) {
  const size_t pairs = (size_t)rows * n;
  count.Reserve((size_t)rows * 4);
  idx.Reserve(pairs * 4);
  post.Reserve(pairs * 4);
  logsum.Reserve((size_t)rows * 4);
  if (with_slot_post) slot_post.Reserve(pairs * 4);
  EventTimer tm(device_ms3 != nullptr, 4);
  UbmFullArgs a;
  Scores(full, host_feats, host_gselect, rows, n, &a, &tm);
  a.min_post = min_post;
  a.out_count = count.as<int32_t>();
  a.out_idx = idx.as<int32_t>();
  a.out_post = post.as<float>();
  a.out_logsum = logsum.as<float>();
  a.out_slot_post = with_slot_post ? slot_post.as<float>() : nullptr;
  Check(launch_ubm_post(a, nullptr), "ubm_post launch");
  tm.Mark();
  if (device_ms3)
    for (int i = 0; i < 3; ++i) device_ms3[i] += tm.Span(i);
}

void UbmPost(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* gselect, int n, float min_post,
             int32_t* count, int32_t* idx, float* post, float* ll, float* logsum, float* device_ms3) {
  if (device_ms3) device_ms3[0] = device_ms3[1] = device_ms3[2] = 0.f;
  const UbmModel::Impl& I = *full.impl_;
  if (!I.full) throw KioError("gselect-to-post: the model is a diagonal one; the posteriors take a full-covariance model");
  const int64_t rows = CheckOffsets("gselect-to-post", row_off, n_utts);
  CheckUbmSelection("gselect-to-post", full, nullptr, 0, n);   // n before the buffers ...
  if (rows == 0) return;
  if (!feats || !gselect || !count || !idx || !post) throw KioError("gselect-to-post: null buffer");
  CheckUbmSelection("gselect-to-post", full, gselect, rows, n);   // ... and the entries last
  UseDevice(I.device, kWhoNeeds);
  // A call's frames go through in parts: the sort's (Gaussian, chunk) table stays small.  A frame's results do not depend on
  // the part it is in.
  constexpr int64_t kPart = 1 << 16;
  UbmPostDevice dev;
  for (int64_t r0 = 0; r0 < rows; r0 += kPart) {
    const int64_t nr = rows - r0 < kPart ? rows - r0 : kPart;
    const size_t pairs = (size_t)nr * n;
    dev.Run(full, feats + (size_t)r0 * I.dim, gselect + (size_t)r0 * n, nr, n, min_post, false, device_ms3);
    dev.count.Download(count + r0, (size_t)nr * 4, "copy the posterior counts");
    dev.idx.Download(idx + (size_t)r0 * n, pairs * 4, "copy the posterior indices");
    dev.post.Download(post + (size_t)r0 * n, pairs * 4, "copy the posteriors");
    if (ll) dev.ll.Download(ll + (size_t)r0 * n, pairs * 4, "copy the log-likelihoods");
    if (logsum) dev.logsum.Download(logsum + r0, (size_t)nr * 4, "copy the log-sums");
  }
}

}  // namespace xv
