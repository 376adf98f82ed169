#include "ivex_train.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <sstream>
#include <thread>

#include "device.h"
#include "ivex_kernels.h"
#include "ivex_train_kernels.h"
#include "plda.h"
#include "ubm_train.h"
#include "ubm_train_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "i-vector extractor training needs";

size_t Tri(int d) { return (size_t)d * (d + 1) / 2; }

void UnpackSym(const double* p, int d, double* a) {
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) a[(size_t)i * d + j] = a[(size_t)j * d + i] = p[Tri(i) + j];
}

// log det of a symmetric positive definite matrix; false if it is not
bool LogDetSym(int n, const double* a, double* logdet) {
  std::vector<double> l((size_t)n * n);
  if (!Cholesky(n, a, l.data())) return false;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += log(l[(size_t)i * n + i]);
  *logdet = 2.0 * s;
  return true;
}

// c [m][n] = a [m][k] b [k][n]
void MatMul(int m, int k, int n, const double* a, const double* b, double* c) {
  for (int i = 0; i < m; ++i) {
    double* ci = c + (size_t)i * n;
    for (int j = 0; j < n; ++j) ci[j] = 0.0;
    for (int q = 0; q < k; ++q) {
      const double av = a[(size_t)i * k + q];
      const double* bq = b + (size_t)q * n;
      for (int j = 0; j < n; ++j) ci[j] += av * bq[j];
    }
  }
}

// f(g) for g in [0, n) on num_threads threads, Gaussian g on thread g mod num_threads; the first exception is rethrown
template <typename F>
void ParallelFor(int n, int num_threads, F f) {
  const int nt = std::max(1, std::min(num_threads, n));
  if (nt == 1) {
    for (int g = 0; g < n; ++g) f(g);
    return;
  }
  std::vector<std::thread> th;
  std::vector<std::string> err((size_t)nt);
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      try {
        for (int g = t; g < n; g += nt) f(g);
      } catch (const std::exception& e) {
        err[t] = e.what();
        if (err[t].empty()) err[t] = "error";
      }
    });
  for (auto& t : th) t.join();
  for (const std::string& e : err)
    if (!e.empty()) throw KioError(e);
}

void ReadDoubles(Input& in, bool binary, const char* tok, size_t n, std::vector<double>* v) {
  ExpectToken(in, binary, tok);
  ReadVectorDouble(in, binary, v);
  if (v->size() != n) throw KioError(std::string(tok) + " has " + std::to_string(v->size()) + " values, the shape asks for " + std::to_string(n));
}

void WriteDoubles(Output& out, bool binary, const char* tok, const std::vector<double>& v) {
  if (v.size() > (size_t)INT32_MAX) throw KioError(std::string(tok) + " has more than 2^31 values");
  WriteToken(out, binary, tok);
  WriteVectorDouble(out, binary, v.data(), (int)v.size());
}

uint64_t Mix(uint64_t seed, uint64_t counter) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + counter;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z >> 11;
}

}  // namespace

uint64_t Mix53(uint64_t seed, uint64_t counter) { return Mix(seed, counter); }

// ---------------------------------------------------------------------------------------------------------------------------------
void IvexStats::Init(int g, int d, int s, bool var) {
  if (g < 1 || d < 1 || s < 1) throw KioError("i-vector extractor statistics: bad shape");
  if (s > kIvexMaxS) throw KioError("the i-vector dimension " + std::to_string(s) + " is above the limit of " + std::to_string(kIvexMaxS));
  if (d > kIvexMaxDim) throw KioError("the feature dimension " + std::to_string(d) + " is above the limit of " + std::to_string(kIvexMaxDim));
  G = g;
  D = d;
  S = s;
  has_variances = var;
  num_ivectors = auxf = frames = 0.0;
  gamma.assign((size_t)g, 0.0);
  Y.assign((size_t)g * d * s, 0.0);
  R.assign((size_t)g * Tri(s), 0.0);
  Sg.assign(var ? (size_t)g * Tri(d) : 0, 0.0);
  ivector_sum.assign((size_t)s, 0.0);
  ivector_scatter.assign(Tri(s), 0.0);
}

void IvexStats::Add(const IvexStats& o) {
  if (o.G != G || o.D != D || o.S != S || o.has_variances != has_variances)
    throw KioError("statistics of " + std::to_string(o.G) + " Gaussians, feature dimension " + std::to_string(o.D) + ", i-vector dimension " +
                   std::to_string(o.S) + (o.has_variances ? " with" : " without") + " variance statistics cannot be added to ones of " +
                   std::to_string(G) + ", " + std::to_string(D) + ", " + std::to_string(S) + (has_variances ? " with" : " without"));
  num_ivectors += o.num_ivectors;
  auxf += o.auxf;
  frames += o.frames;
  auto add = [](std::vector<double>& a, const std::vector<double>& b) {
    for (size_t i = 0; i < a.size(); ++i) a[i] += b[i];
  };
  add(gamma, o.gamma);
  add(Y, o.Y);
  add(R, o.R);
  add(Sg, o.Sg);
  add(ivector_sum, o.ivector_sum);
  add(ivector_scatter, o.ivector_scatter);
}

void ReadIvexStatsFile(const std::string& rxfilename, IvexStats* s) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ExpectToken(in, binary, "<IvectorExtractorStats>");
  ExpectToken(in, binary, "<NumGauss>");
  const int G = ReadInt32(in, binary);
  ExpectToken(in, binary, "<FeatDim>");
  const int D = ReadInt32(in, binary);
  ExpectToken(in, binary, "<IvectorDim>");
  const int S = ReadInt32(in, binary);
  ExpectToken(in, binary, "<HasVariances>");
  const bool var = ReadBool(in, binary);
  if (G < 1 || G > (1 << 24)) throw KioError("bad number of Gaussians " + std::to_string(G) + " in " + rxfilename);
  s->Init(G, D, S, var);
  ExpectToken(in, binary, "<NumIvectors>");
  s->num_ivectors = ReadFloatOrDouble(in, binary);
  ExpectToken(in, binary, "<Auxf>");
  s->auxf = ReadFloatOrDouble(in, binary);
  ExpectToken(in, binary, "<Frames>");
  s->frames = ReadFloatOrDouble(in, binary);
  ReadDoubles(in, binary, "<gamma>", (size_t)G, &s->gamma);
  ReadDoubles(in, binary, "<Y>", (size_t)G * D * S, &s->Y);
  ReadDoubles(in, binary, "<R>", (size_t)G * Tri(S), &s->R);
  if (var) ReadDoubles(in, binary, "<S>", (size_t)G * Tri(D), &s->Sg);
  ReadDoubles(in, binary, "<IvectorSum>", (size_t)S, &s->ivector_sum);
  ReadDoubles(in, binary, "<IvectorScatter>", Tri(S), &s->ivector_scatter);
  ExpectToken(in, binary, "</IvectorExtractorStats>");
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
}

void WriteIvexStatsFile(const std::string& wxfilename, bool binary, const IvexStats& s) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteToken(out, binary, "<IvectorExtractorStats>");
  WriteToken(out, binary, "<NumGauss>");
  WriteInt32(out, binary, s.G);
  WriteToken(out, binary, "<FeatDim>");
  WriteInt32(out, binary, s.D);
  WriteToken(out, binary, "<IvectorDim>");
  WriteInt32(out, binary, s.S);
  WriteToken(out, binary, "<HasVariances>");
  WriteBool(out, binary, s.has_variances);
  WriteToken(out, binary, "<NumIvectors>");
  WriteDouble(out, binary, s.num_ivectors);
  WriteToken(out, binary, "<Auxf>");
  WriteDouble(out, binary, s.auxf);
  WriteToken(out, binary, "<Frames>");
  WriteDouble(out, binary, s.frames);
  WriteDoubles(out, binary, "<gamma>", s.gamma);
  WriteDoubles(out, binary, "<Y>", s.Y);
  WriteDoubles(out, binary, "<R>", s.R);
  if (s.has_variances) WriteDoubles(out, binary, "<S>", s.Sg);
  WriteDoubles(out, binary, "<IvectorSum>", s.ivector_sum);
  WriteDoubles(out, binary, "<IvectorScatter>", s.ivector_scatter);
  WriteToken(out, binary, "</IvectorExtractorStats>");
  if (!binary) out.Put('\n');
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

// ---------------------------------------------------------------------------------------------------------------------------------
void IvexInit(const FullGmmData& ubm, int S, uint64_t seed, IvexData* out) {
  const int G = ubm.num_gauss, D = ubm.dim;
  if (G < 1 || D < 1 || ubm.weights.size() != (size_t)G || ubm.means_invcovars.size() != (size_t)G * D || ubm.inv_covars.size() != (size_t)G * Tri(D))
    throw KioError("ivector-extractor-init: the UBM's arrays do not have its shape");
  if (S < 1 || S > kIvexMaxS)
    throw KioError("the i-vector dimension " + std::to_string(S) + " is outside [1, " + std::to_string(kIvexMaxS) + "], the device solve's limit");
  if (D > kIvexMaxDim)
    throw KioError("the UBM's feature dimension " + std::to_string(D) + " is above the device kernels' limit of " + std::to_string(kIvexMaxDim));
  *out = IvexData();
  out->G = G;
  out->D = D;
  out->S = S;
  out->prior_offset = kIvexInitPriorOffset;
  out->w_vec.assign(ubm.weights.begin(), ubm.weights.end());
  out->sigma_inv.assign(ubm.inv_covars.begin(), ubm.inv_covars.end());
  out->M.resize((size_t)G * D * S);
  const double two_pi = 6.283185307179586476925286766559;
  for (size_t e = 0; e < out->M.size(); ++e) {
    const double u1 = ((double)Mix(seed, 2 * e) + 1.0) / 9007199254740992.0, u2 = (double)Mix(seed, 2 * e + 1) / 9007199254740992.0;
    out->M[e] = sqrt(-2.0 * log(u1)) * cos(two_pi * u2);
  }
  std::vector<double> inv((size_t)D * D), sig((size_t)D * D);
  for (int g = 0; g < G; ++g) {
    UnpackSym(out->sigma_inv.data() + (size_t)g * Tri(D), D, inv.data());
    if (!InvertSymmetric(D, inv.data(), sig.data()))
      throw KioError("the inverse covariance of component " + std::to_string(g) + " of the UBM is not positive definite");
    for (int i = 0; i < D; ++i) {
      double s = 0.0;
      for (int j = 0; j < D; ++j) s += sig[(size_t)i * D + j] * (double)ubm.means_invcovars[(size_t)g * D + j];
      out->M[((size_t)g * D + i) * S] = s / kIvexInitPriorOffset;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
void IvexEst(const IvexStats& st, const IvexEstOptions& o, IvexData* model, IvexEstResult* res) {
  const int G = model->G, D = model->D, S = model->S;
  const size_t P = Tri(S), TD = Tri(D), DS = (size_t)D * S, SS = (size_t)S * S, DD = (size_t)D * D;
  if (st.G != G || st.D != D || st.S != S)
    throw KioError("the statistics (" + std::to_string(st.G) + " Gaussians, feature dimension " + std::to_string(st.D) + ", i-vector dimension " +
                   std::to_string(st.S) + ") are not the model's (" + std::to_string(G) + ", " + std::to_string(D) + ", " + std::to_string(S) + ")");
  if (model->M.size() != (size_t)G * DS || model->sigma_inv.size() != (size_t)G * TD || model->w_vec.size() != (size_t)G)
    throw KioError("i-vector extractor: the arrays do not have the model's shape");
  if (!(st.num_ivectors >= 1.0)) throw KioError("the statistics hold no i-vector: nothing to estimate from");
  *res = IvexEstResult();
  double frames = 0.0;
  for (int g = 0; g < G; ++g) frames += st.gamma[g];
  if (!(frames > 0.0)) throw KioError("the statistics hold no frame: nothing to estimate from");
  std::vector<char> updated((size_t)G, 0);
  std::vector<int> eig_floored((size_t)G, 0), var_floored((size_t)G, 0);
  std::vector<double> impr_proj((size_t)G, 0.0), impr_var((size_t)G, 0.0);
  std::vector<double> MR((size_t)G * DS);   // M_g R_g with the new M_g
  for (int g = 0; g < G; ++g)
    if (st.gamma[g] >= o.gaussian_min_count) {
      updated[g] = 1;
      ++res->gauss_updated;
    } else {
      ++res->gauss_skipped;
      std::ostringstream msg;
      msg << "Skipping Gaussian index " << g << " because count " << st.gamma[g] << " is below min-count.";
      res->warnings.push_back(msg.str());
    }

  // 1. the projections
  ParallelFor(G, o.num_threads, [&](int g) {
    if (!updated[g]) return;
    std::vector<double> Rg(SS), lam((size_t)S), U(SS), Rinv(SS), sinv(DD), sim(DS), mr(DS), resid(DS), delta(DS);
    UnpackSym(st.R.data() + (size_t)g * P, S, Rg.data());
    SymmetricEig(S, Rg.data(), lam.data(), U.data());
    double lmax = 0.0;
    for (int k = 0; k < S; ++k) lmax = std::max(lmax, lam[k]);
    const double floor = std::max(1e-40, lmax / 1e4);
    for (int k = 0; k < S; ++k)
      if (lam[k] < floor) {
        lam[k] = floor;
        ++eig_floored[g];
      }
    for (int i = 0; i < S; ++i)
      for (int j = 0; j <= i; ++j) {
        double v = 0.0;
        for (int k = 0; k < S; ++k) v += U[(size_t)i * S + k] / lam[k] * U[(size_t)j * S + k];
        Rinv[(size_t)i * S + j] = Rinv[(size_t)j * S + i] = v;
      }
    double* M = model->M.data() + (size_t)g * DS;
    const double* Y = st.Y.data() + (size_t)g * DS;
    UnpackSym(model->sigma_inv.data() + (size_t)g * TD, D, sinv.data());
    auto objf = [&](const double* m, const double* m_r) {
      MatMul(D, D, S, sinv.data(), m, sim.data());
      double a = 0.0, b = 0.0;
      for (size_t e = 0; e < DS; ++e) {
        a += sim[e] * Y[e];
        b += sim[e] * m_r[e];
      }
      return a - 0.5 * b;
    };
    MatMul(D, S, S, M, Rg.data(), mr.data());
    const double before = objf(M, mr.data());
    for (size_t e = 0; e < DS; ++e) resid[e] = Y[e] - mr[e];
    MatMul(D, S, S, resid.data(), Rinv.data(), delta.data());
    for (size_t e = 0; e < DS; ++e) M[e] += delta[e];
    double* mr_new = MR.data() + (size_t)g * DS;
    MatMul(D, S, S, M, Rg.data(), mr_new);
    impr_proj[g] = objf(M, mr_new) - before;
  });
  for (int g = 0; g < G; ++g) {
    res->eig_floored += eig_floored[g];
    res->impr_proj += impr_proj[g];
  }
  res->impr_proj /= frames;

  // 2. the variances
  if (st.has_variances) {
    if (st.Sg.size() != (size_t)G * TD) throw KioError("the statistics' second-order term does not have the model's shape");
    std::vector<double> raw((size_t)G * DD, 0.0);
    ParallelFor(G, o.num_threads, [&](int g) {
      if (!updated[g]) return;
      const double* M = model->M.data() + (size_t)g * DS;
      const double* Y = st.Y.data() + (size_t)g * DS;
      const double* mr = MR.data() + (size_t)g * DS;
      const double* sg = st.Sg.data() + (size_t)g * TD;
      double* r = raw.data() + (size_t)g * DD;
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
          double ym = 0.0, mrm = 0.0;
          for (int s = 0; s < S; ++s) {
            ym += Y[(size_t)i * S + s] * M[(size_t)j * S + s] + M[(size_t)i * S + s] * Y[(size_t)j * S + s];
            mrm += mr[(size_t)i * S + s] * M[(size_t)j * S + s];
          }
          r[(size_t)i * D + j] = r[(size_t)j * D + i] = sg[Tri(i) + j] - ym + mrm;
        }
    });
    std::vector<double> F(DD, 0.0), L(DD), Linv(DD);
    double count = 0.0;
    for (int g = 0; g < G; ++g) {
      if (!updated[g]) continue;
      count += st.gamma[g];
      for (size_t e = 0; e < DD; ++e) F[e] += raw[(size_t)g * DD + e];
    }
    if (res->gauss_updated > 0) {
      for (size_t e = 0; e < DD; ++e) F[e] *= o.variance_floor_factor / count;
      if (!Cholesky(D, F.data(), L.data())) throw KioError("the variance floor matrix is not positive definite: too little data, or a floor factor of 0");
      InvertLower(D, L.data(), Linv.data());
    }
    ParallelFor(G, o.num_threads, [&](int g) {
      if (!updated[g]) return;
      std::vector<double> sig(DD), t1(DD), t2(DD), ev((size_t)D), W(DD), inv(DD), old(DD);
      const double* r = raw.data() + (size_t)g * DD;
      const double gam = st.gamma[g];
      for (size_t e = 0; e < DD; ++e) sig[e] = r[e] / gam;
      MatMul(D, D, D, Linv.data(), sig.data(), t1.data());
      for (int i = 0; i < D; ++i)   // t2 = t1 Linv', symmetric
        for (int j = 0; j <= i; ++j) {
          double v = 0.0;
          for (int k = 0; k < D; ++k) v += t1[(size_t)i * D + k] * Linv[(size_t)j * D + k];
          t2[(size_t)i * D + j] = t2[(size_t)j * D + i] = v;
        }
      SymmetricEig(D, t2.data(), ev.data(), W.data());
      for (int k = 0; k < D; ++k)
        if (ev[k] < 1.0) {
          ev[k] = 1.0;
          ++var_floored[g];
        }
      MatMul(D, D, D, L.data(), W.data(), t1.data());   // L W
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
          double v = 0.0;
          for (int k = 0; k < D; ++k) v += t1[(size_t)i * D + k] * ev[k] * t1[(size_t)j * D + k];
          sig[(size_t)i * D + j] = sig[(size_t)j * D + i] = v;
        }
      if (!InvertSymmetric(D, sig.data(), inv.data()))
        throw KioError("the new covariance of Gaussian " + std::to_string(g) + " is not positive definite after flooring");
      double* packed = model->sigma_inv.data() + (size_t)g * TD;
      UnpackSym(packed, D, old.data());
      auto objf = [&](const double* si) {
        double tr = 0.0, ld = 0.0;
        for (size_t e = 0; e < DD; ++e) tr += si[e] * r[e];
        if (!LogDetSym(D, si, &ld)) throw KioError("the inverse covariance of Gaussian " + std::to_string(g) + " is not positive definite");
        return -0.5 * tr + 0.5 * gam * ld;
      };
      impr_var[g] = objf(inv.data()) - objf(old.data());
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) packed[Tri(i) + j] = inv[(size_t)i * D + j];
    });
    for (int g = 0; g < G; ++g) {
      res->var_floored += var_floored[g];
      res->var_floored_gauss += var_floored[g] ? 1 : 0;
      res->impr_var += impr_var[g];
    }
    res->impr_var /= frames;
  }

  // 3. the prior
  const double n = st.num_ivectors, p = model->prior_offset;
  std::vector<double> mu((size_t)S), C(SS), s((size_t)S), Pm(SS), T(SS), Tinv(SS), v((size_t)S), a((size_t)S, 0.0);
  for (int i = 0; i < S; ++i) mu[i] = st.ivector_sum[i] / n;
  for (int i = 0; i < S; ++i)
    for (int j = 0; j <= i; ++j) C[(size_t)i * S + j] = C[(size_t)j * S + i] = st.ivector_scatter[Tri(i) + j] / n - mu[i] * mu[j];
  SymmetricEig(S, C.data(), s.data(), Pm.data());
  double tr_c = 0.0, dist = 0.0, logdet_c = 0.0;
  for (int i = 0; i < S; ++i) {
    tr_c += C[(size_t)i * S + i];
    const double d = mu[i] - (i == 0 ? p : 0.0);
    dist += d * d;
  }
  for (int k = 0; k < S; ++k) {
    if (s[k] < 1e-7) {
      s[k] = 1e-7;
      ++res->prior_floored;
    }
    logdet_c += log(s[k]);
  }
  res->impr_prior = n * (-0.5 * (logdet_c + S) + 0.5 * (tr_c + dist)) / frames;
  for (int i = 0; i < S; ++i)
    for (int j = 0; j < S; ++j) {
      T[(size_t)i * S + j] = Pm[(size_t)j * S + i] / sqrt(s[i]);
      Tinv[(size_t)i * S + j] = Pm[(size_t)i * S + j] * sqrt(s[j]);
    }
  double vnorm = 0.0;
  for (int i = 0; i < S; ++i) {
    double t = 0.0;
    for (int j = 0; j < S; ++j) t += T[(size_t)i * S + j] * mu[j];
    v[i] = t;
    vnorm += t * t;
  }
  vnorm = sqrt(vnorm);
  if (!(vnorm > 0.0) || !std::isfinite(vnorm)) throw KioError("the mean of the i-vectors is zero or not finite: the prior cannot be updated");
  double anorm = 0.0;
  for (int i = 0; i < S; ++i) {
    a[i] = v[i] / vnorm - (i == 0 ? 1.0 : 0.0);
    anorm += a[i] * a[i];
  }
  anorm = sqrt(anorm);
  if (anorm > 0.0)
    for (int i = 0; i < S; ++i) a[i] /= anorm;
  // V = H T, V^-1 = T^-1 H, H = I - 2 a a'
  std::vector<double> V(SS), Vinv(SS), tmp((size_t)S);
  for (int j = 0; j < S; ++j) {
    double t = 0.0;
    for (int k = 0; k < S; ++k) t += a[k] * T[(size_t)k * S + j];
    tmp[j] = t;
  }
  for (int i = 0; i < S; ++i)
    for (int j = 0; j < S; ++j) V[(size_t)i * S + j] = T[(size_t)i * S + j] - 2.0 * a[i] * tmp[j];
  for (int i = 0; i < S; ++i) {
    double t = 0.0;
    for (int k = 0; k < S; ++k) t += Tinv[(size_t)i * S + k] * a[k];
    for (int j = 0; j < S; ++j) Vinv[(size_t)i * S + j] = Tinv[(size_t)i * S + j] - 2.0 * t * a[j];
  }
  if (o.diagonalize && S > 1) {
    // Uavg = sum_g w_g M_g' Sigma_g^-1 M_g, rows dealt over the threads, g ascending in every element
    std::vector<double> sim_all((size_t)G * DS), Uavg(SS, 0.0);
    ParallelFor(G, o.num_threads, [&](int g) {
      std::vector<double> sinv(DD);
      UnpackSym(model->sigma_inv.data() + (size_t)g * TD, D, sinv.data());
      MatMul(D, D, S, sinv.data(), model->M.data() + (size_t)g * DS, sim_all.data() + (size_t)g * DS);
    });
    ParallelFor(S, o.num_threads, [&](int r) {
      double* row = Uavg.data() + (size_t)r * S;
      for (int g = 0; g < G; ++g) {
        const double w = model->w_vec[g];
        const double* M = model->M.data() + (size_t)g * DS;
        const double* sim = sim_all.data() + (size_t)g * DS;
        for (int d = 0; d < D; ++d) {
          const double m = w * M[(size_t)d * S + r];
          for (int c = 0; c < S; ++c) row[c] += m * sim[(size_t)d * S + c];
        }
      }
    });
    std::vector<double> t1(SS), A(SS);
    MatMul(S, S, S, Uavg.data(), Vinv.data(), t1.data());
    for (int i = 0; i < S; ++i)   // A = Vinv' t1
      for (int j = 0; j < S; ++j) {
        double t = 0.0;
        for (int k = 0; k < S; ++k) t += Vinv[(size_t)k * S + i] * t1[(size_t)k * S + j];
        A[(size_t)i * S + j] = t;
      }
    const int S1 = S - 1;
    std::vector<double> Bm((size_t)S1 * S1), be((size_t)S1), E((size_t)S1 * S1);
    for (int i = 0; i < S1; ++i)
      for (int j = 0; j <= i; ++j)
        Bm[(size_t)i * S1 + j] = Bm[(size_t)j * S1 + i] = 0.5 * (A[(size_t)(i + 1) * S + j + 1] + A[(size_t)(j + 1) * S + i + 1]);
    SymmetricEig(S1, Bm.data(), be.data(), E.data());
    // V <- Rot V, Vinv <- Vinv Rot', Rot = diag(1, E')
    std::vector<double> V2(V), Vi2(Vinv);
    for (int i = 0; i < S1; ++i)
      for (int j = 0; j < S; ++j) {
        double t = 0.0;
        for (int k = 0; k < S1; ++k) t += E[(size_t)k * S1 + i] * V[(size_t)(k + 1) * S + j];
        V2[(size_t)(i + 1) * S + j] = t;
      }
    for (int i = 0; i < S; ++i)
      for (int j = 0; j < S1; ++j) {
        double t = 0.0;
        for (int k = 0; k < S1; ++k) t += Vinv[(size_t)i * S + k + 1] * E[(size_t)k * S1 + j];
        Vi2[(size_t)i * S + j + 1] = t;
      }
    V.swap(V2);
    Vinv.swap(Vi2);
  }
  ParallelFor(G, o.num_threads, [&](int g) {
    std::vector<double> m(DS);
    double* M = model->M.data() + (size_t)g * DS;
    MatMul(D, S, S, M, Vinv.data(), m.data());
    std::copy(m.begin(), m.end(), M);
  });
  model->prior_offset = vnorm;
  res->V.swap(V);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct IvexAccumulator::Impl {
  IvexModel* model = nullptr;
  int G = 0, D = 0, S = 0;
  int64_t P = 0, K = 0;
  bool update_variances = false, compute_auxf = false;
  int pending = 0;
  double accepted = 0.0;
  DevBuf p_gamma, p_X, p_m, p_scatter, p_logdet, p_auxf, zwork;   // the pending slots
  DevBuf gamma, Y, R, ivector_sum, ivector_scatter, auxf;         // the running accumulators
  std::unique_ptr<FgmmAccumulator> second;                        // S_g, through the UBM-training path
  // frames of accepted utterances that do not fill a block yet
  std::vector<float> f_feats, f_w;
  std::vector<int32_t> f_count, f_idx;
  bool timed = false;
  float ms3[3] = {0.f, 0.f, 0.f};

  void Flush() {
    if (pending == 0) return;
    IvexRankUpdateArgs r;
    memset(&r, 0, sizeof r);
    r.A = p_gamma.as<double>();
    r.B = p_scatter.as<double>();
    r.C = R.as<double>();
    r.count = pending;
    r.M = G;
    r.N = r.ldc = P;
    IvexRankUpdateArgs y;
    memset(&y, 0, sizeof y);
    y.A = p_X.as<double>();
    y.B = p_m.as<double>();
    y.C = Y.as<double>();
    y.count = pending;
    y.M = K;
    y.N = y.ldc = S;
    IvexSmallSumsArgs s;
    memset(&s, 0, sizeof s);
    s.count = pending;
    s.G = G;
    s.S = S;
    s.p_gamma = p_gamma.as<double>();
    s.p_m = p_m.as<double>();
    s.p_scatter = p_scatter.as<double>();
    s.p_auxf = p_auxf.as<double>();
    s.gamma = gamma.as<double>();
    s.ivector_sum = ivector_sum.as<double>();
    s.ivector_scatter = ivector_scatter.as<double>();
    s.auxf = auxf.as<double>();
    EventTimer tm(timed, 3);
    tm.Mark();
    Check(launch_ivex_rank_update(r, nullptr), "ivex_rank_update launch (R)");
    tm.Mark();
    Check(launch_ivex_rank_update(y, nullptr), "ivex_rank_update launch (Y)");
    tm.Mark();
    Check(launch_ivex_small_sums(s, nullptr), "ivex_small_sums launch");
    if (timed) {
      ms3[1] += tm.Span(0);
      ms3[2] += tm.Span(1);
    }
    pending = 0;
  }

  void Group(const IvexGroupView& v) {
    int i = 0;
    while (i < v.B) {
      IvexPosteriorArgs a;
      memset(&a, 0, sizeof a);
      int n = 0;
      for (; i < v.B && pending + n < kIvexTrainSlots; ++i)
        if (v.status[i] == 0) {
          a.src[n] = (uint8_t)i;
          a.slot[n] = (uint8_t)(pending + n);
          ++n;
        }
      if (n > 0) {
        a.n = n;
        a.G = G;
        a.D = D;
        a.S = S;
        a.prior_offset = model->prior_offset();
        a.gamma = v.gamma;
        a.X = v.X;
        a.linear = v.linear;
        a.quadratic = v.quadratic;
        a.work = v.work;
        a.solution = v.solution;
        a.zwork = zwork.as<double>();
        a.p_gamma = p_gamma.as<double>();
        a.p_X = p_X.as<double>();
        a.p_m = p_m.as<double>();
        a.p_scatter = p_scatter.as<double>();
        a.p_logdet = p_logdet.as<double>();
        a.p_auxf = p_auxf.as<double>();
        EventTimer tm(timed);
        tm.Start();
        Check(launch_ivex_posterior(a, nullptr), "ivex_posterior launch");
        if (timed) ms3[0] += tm.Stop();
        pending += n;
        accepted += n;
      }
      if (pending == kIvexTrainSlots) Flush();
    }
  }

  // whole blocks of the pending frames, or with `all` everything, through the second-moment accumulator.  FgmmAccAdd is called
  // whole, as fgmm-global-acc-stats's caller-held-posterior path: the device path of ubm_train.cc is reused, not factored.  The
  // price is that the frames IvexExtract already uploaded are staged on the host (at most a block and an utterance of them) and
  // uploaded a second time, because a block is cut from accepted utterances only and may straddle launch groups and calls.
  // Feeding the accumulator from the group's device buffers is a follow-up; the staging is in profiles/ivex_train_bench.md.
  void FlushFrames(bool all) {
    if (!second) return;
    const size_t rows = f_count.size();
    size_t r0 = 0, pair0 = 0;
    std::vector<int32_t> off;
    while (r0 < rows && (rows - r0 >= (size_t)kFgmmAccFrameBlock || all)) {
      const size_t nr = std::min(rows - r0, (size_t)kFgmmAccFrameBlock);
      off.assign(1, 0);
      for (size_t t = 0; t < nr; ++t) off.push_back(off.back() + f_count[r0 + t]);
      FgmmAccAdd(second.get(), f_feats.data() + r0 * D, (int64_t)nr, off.data(), f_idx.data() + pair0, f_w.data() + pair0);
      pair0 += (size_t)off.back();
      r0 += nr;
    }
    f_feats.erase(f_feats.begin(), f_feats.begin() + r0 * D);
    f_count.erase(f_count.begin(), f_count.begin() + r0);
    f_idx.erase(f_idx.begin(), f_idx.begin() + pair0);
    f_w.erase(f_w.begin(), f_w.begin() + pair0);
  }
};

IvexAccumulator::~IvexAccumulator() {}

IvexAccumulator* IvexAccCreate(IvexModel* model, bool update_variances, bool compute_auxf) {
  if (!model) throw KioError("i-vector extractor accumulator: no model");
  UseDevice(model->device(), kWhoNeeds);
  std::unique_ptr<IvexAccumulator> h(new IvexAccumulator);
  h->impl_.reset(new IvexAccumulator::Impl);
  IvexAccumulator::Impl& I = *h->impl_;
  I.model = model;
  I.G = model->num_gauss();
  I.D = model->feat_dim();
  I.S = model->ivector_dim();
  I.P = (int64_t)Tri(I.S);
  I.K = (int64_t)I.G * I.D;
  I.update_variances = update_variances;
  I.compute_auxf = compute_auxf;
  const size_t slots = kIvexTrainSlots;
  I.p_gamma.Alloc(slots * I.G * 8);
  I.p_X.Alloc(slots * (size_t)I.K * 8);
  I.p_m.Alloc(slots * I.S * 8);
  I.p_scatter.Alloc(slots * (size_t)I.P * 8);
  I.p_logdet.Alloc(slots * 8);
  I.p_auxf.Alloc(slots * 8);
  I.zwork.Alloc(slots * (size_t)I.S * I.S * 8);
  I.gamma.Alloc((size_t)I.G * 8);
  I.Y.Alloc((size_t)I.K * I.S * 8);
  I.R.Alloc((size_t)I.G * I.P * 8);
  I.ivector_sum.Alloc((size_t)I.S * 8);
  I.ivector_scatter.Alloc((size_t)I.P * 8);
  I.auxf.Alloc(8);
  for (DevBuf* b : {&I.gamma, &I.Y, &I.R, &I.ivector_sum, &I.ivector_scatter, &I.auxf}) Check(hipMemset(b->p, 0, b->cap), "hipMemset");
  if (update_variances) I.second.reset(FgmmAccCreate(model->device(), I.G, I.D, kFgmmFlagVariances));
  return h.release();
}

void IvexAccAdd(IvexAccumulator* acc, const float* feats, const int32_t* row_off, int n_utts, const int32_t* post_off, const int32_t* post_idx,
                const float* post_w, int32_t* status, float* device_ms3) {
  IvexAccumulator::Impl& I = *acc->impl_;
  I.timed = device_ms3 != nullptr;
  I.ms3[0] = I.ms3[1] = I.ms3[2] = 0.f;
  if (n_utts < 0) throw KioError("i-vector extractor accumulator: bad argument");
  std::vector<float> iv((size_t)std::max(n_utts, 1) * I.S);
  std::vector<int32_t> st((size_t)std::max(n_utts, 1), 0);
  IvexOutputs out;
  out.ivectors = iv.data();
  out.status = st.data();
  const IvexGroupHook hook = [&I](const IvexGroupView& v) { I.Group(v); };
  IvexExtract(*I.model, feats, row_off, n_utts, post_off, post_idx, post_w, 1.0, 0.0, out, &hook);
  if (I.second)
    for (int u = 0; u < n_utts; ++u) {
      if (st[u] != 0) continue;
      const int64_t r0 = row_off[u], r1 = row_off[u + 1];
      I.f_feats.insert(I.f_feats.end(), feats + r0 * I.D, feats + r1 * I.D);
      for (int64_t t = r0; t < r1; ++t) I.f_count.push_back(post_off[t + 1] - post_off[t]);
      I.f_idx.insert(I.f_idx.end(), post_idx + post_off[r0], post_idx + post_off[r1]);
      I.f_w.insert(I.f_w.end(), post_w + post_off[r0], post_w + post_off[r1]);
      I.FlushFrames(false);
    }
  if (status) std::copy(st.begin(), st.begin() + n_utts, status);
  if (device_ms3) std::copy(I.ms3, I.ms3 + 3, device_ms3);
}

void IvexAccGet(IvexAccumulator* acc, IvexStats* out, float* device_ms3) {
  IvexAccumulator::Impl& I = *acc->impl_;
  UseDevice(I.model->device(), kWhoNeeds);
  I.timed = device_ms3 != nullptr;
  I.ms3[0] = I.ms3[1] = I.ms3[2] = 0.f;
  I.Flush();
  I.FlushFrames(true);
  if (device_ms3) std::copy(I.ms3, I.ms3 + 3, device_ms3);
  const int G = I.G, D = I.D, S = I.S;
  out->Init(G, D, S, I.update_variances);
  out->num_ivectors = I.accepted;
  I.gamma.Download(out->gamma.data(), out->gamma.size() * 8, "copy gamma");
  I.Y.Download(out->Y.data(), out->Y.size() * 8, "copy Y");
  I.R.Download(out->R.data(), out->R.size() * 8, "copy R");
  I.ivector_sum.Download(out->ivector_sum.data(), out->ivector_sum.size() * 8, "copy the i-vector sum");
  I.ivector_scatter.Download(out->ivector_scatter.data(), out->ivector_scatter.size() * 8, "copy the i-vector scatter");
  if (I.second) FgmmAccGet(*I.second, nullptr, nullptr, out->Sg.data());
  for (int g = 0; g < I.G; ++g) out->frames += out->gamma[g];
  if (!I.compute_auxf) return;
  double auxf = 0.0;
  I.auxf.Download(&auxf, 8, "copy the objective");
  // the two terms that are linear in the statistics
  const std::vector<double>& w = I.model->w_vec();
  const std::vector<double>& sig = I.model->sigma_inv();
  const size_t TD = Tri(D);
  std::vector<double> full((size_t)D * D);
  const double log_2pi = 1.8378770664093454835606594728112;
  double weight_gconst = 0.0, trace = 0.0;
  for (int g = 0; g < G; ++g) {
    const double gam = out->gamma[g];
    if (gam == 0.0) continue;
    double ld = 0.0;
    UnpackSym(sig.data() + (size_t)g * TD, D, full.data());
    if (!LogDetSym(D, full.data(), &ld)) throw KioError("the inverse covariance of Gaussian " + std::to_string(g) + " is not positive definite");
    weight_gconst += gam * (log(w[g]) - 0.5 * (D * log_2pi - ld));
    if (I.update_variances) {
      const double* c = out->Sg.data() + (size_t)g * TD;
      const double* s = sig.data() + (size_t)g * TD;
      double tr = 0.0;
      for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) tr += (i == j ? 1.0 : 2.0) * c[Tri(i) + j] * s[Tri(i) + j];
      trace += tr;
    } else {
      trace += gam * D;
    }
  }
  out->auxf = auxf + weight_gconst - 0.5 * trace;
}

int IvexAccPending(IvexAccumulator* acc, double* m, double* scatter, double* logdet, double* auxf) {
  IvexAccumulator::Impl& I = *acc->impl_;
  UseDevice(I.model->device(), kWhoNeeds);
  const size_t n = (size_t)I.pending;
  if (m) I.p_m.Download(m, n * I.S * 8, "copy the pending solutions");
  if (scatter) I.p_scatter.Download(scatter, n * (size_t)I.P * 8, "copy the pending scatters");
  if (logdet) I.p_logdet.Download(logdet, n * 8, "copy the pending log-determinants");
  if (auxf) I.p_auxf.Download(auxf, n * 8, "copy the pending objectives");
  return I.pending;
}

void IvexRankUpdateHost(int device, const double* A, const double* B, double* C, int slots, int64_t M, int64_t N, int64_t c_rows, int64_t ldc) {
  if (!A || !B || !C || slots < 0 || slots > kIvexTrainSlots || M < 1 || N < 1 || c_rows < M || ldc < N)
    throw KioError("rank update: 0 <= slots <= " + std::to_string(kIvexTrainSlots) + ", M >= 1, N >= 1, c_rows >= M and ldc >= N are required");
  UseDevice(device, kWhoNeeds);
  DevBuf dA, dB, dC;
  dA.Upload(A, (size_t)kIvexTrainSlots * M * 8, "copy A");
  dB.Upload(B, (size_t)kIvexTrainSlots * N * 8, "copy B");
  dC.Upload(C, (size_t)c_rows * ldc * 8, "copy C");
  IvexRankUpdateArgs r;
  memset(&r, 0, sizeof r);
  r.A = dA.as<double>();
  r.B = dB.as<double>();
  r.C = dC.as<double>();
  r.count = slots;
  r.M = M;
  r.N = N;
  r.ldc = ldc;
  Check(launch_ivex_rank_update(r, nullptr), "ivex_rank_update launch");
  Check(hipDeviceSynchronize(), "ivex_rank_update");
  dC.Download(C, (size_t)c_rows * ldc * 8, "copy C");
}

}  // namespace xv
