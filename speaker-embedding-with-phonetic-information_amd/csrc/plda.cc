#include "plda.h"

#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <numeric>
#include <sstream>
#include <string>

#include "device.h"
#include "kio.h"
#include "plda_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "the PLDA back-end kernels need";

using Mat = std::vector<double>;   // row-major n x n

Mat Identity(int n) {
  Mat m((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) m[(size_t)i * n + i] = 1.0;
  return m;
}

// a m a^T for a [r][n], m [n][n] -> [r][r], symmetrised
Mat Sandwich(int r, int n, const Mat& a, const Mat& m) {
  Mat am((size_t)r * n, 0.0);
  for (int i = 0; i < r; ++i)
    for (int k = 0; k < n; ++k) {
      const double x = a[(size_t)i * n + k];
      if (x == 0.0) continue;
      for (int j = 0; j < n; ++j) am[(size_t)i * n + j] += x * m[(size_t)k * n + j];
    }
  Mat out((size_t)r * r);
  for (int i = 0; i < r; ++i)
    for (int j = i; j < r; ++j) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += am[(size_t)i * n + k] * a[(size_t)j * n + k];
      out[(size_t)i * r + j] = out[(size_t)j * r + i] = s;
    }
  return out;
}

// JAMA's tred2 / tql2 (public domain): v holds the matrix on entry, the eigenvectors (columns) on exit.
void Tred2(int n, double* v, double* d, double* e) {
#define V(i, j) v[(size_t)(i) * n + (j)]
  for (int j = 0; j < n; ++j) d[j] = V(n - 1, j);
  for (int i = n - 1; i > 0; --i) {
    double scale = 0.0, h = 0.0;
    for (int k = 0; k < i; ++k) scale += fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (int j = 0; j < i; ++j) {
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
        V(j, i) = 0.0;
      }
    } else {
      for (int k = 0; k < i; ++k) {
        d[k] /= scale;
        h += d[k] * d[k];
      }
      double f = d[i - 1];
      double g = sqrt(h);
      if (f > 0) g = -g;
      e[i] = scale * g;
      h = h - f * g;
      d[i - 1] = f - g;
      for (int j = 0; j < i; ++j) e[j] = 0.0;
      for (int j = 0; j < i; ++j) {
        f = d[j];
        V(j, i) = f;
        g = e[j] + V(j, j) * f;
        for (int k = j + 1; k <= i - 1; ++k) {
          g += V(k, j) * d[k];
          e[k] += V(k, j) * f;
        }
        e[j] = g;
      }
      f = 0.0;
      for (int j = 0; j < i; ++j) {
        e[j] /= h;
        f += e[j] * d[j];
      }
      const double hh = f / (h + h);
      for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (int j = 0; j < i; ++j) {
        f = d[j];
        g = e[j];
        for (int k = j; k <= i - 1; ++k) V(k, j) -= (f * e[k] + g * d[k]);
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  for (int i = 0; i < n - 1; ++i) {
    V(n - 1, i) = V(i, i);
    V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (int k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (int j = 0; j <= i; ++j) {
        double g = 0.0;
        for (int k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (int k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (int k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
  }
  for (int j = 0; j < n; ++j) {
    d[j] = V(n - 1, j);
    V(n - 1, j) = 0.0;
  }
  V(n - 1, n - 1) = 1.0;
  e[0] = 0.0;
}

void Tql2(int n, double* v, double* d, double* e) {
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  double f = 0.0, tst1 = 0.0;
  const double eps = ldexp(1.0, -52);
  for (int l = 0; l < n; ++l) {
    tst1 = std::max(tst1, fabs(d[l]) + fabs(e[l]));
    int m = l;
    while (m < n) {
      if (fabs(e[m]) <= eps * tst1) break;
      ++m;
    }
    if (m == n) m = n - 1;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 200) throw EngineError("symmetric eigensolver did not converge");
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = hypot(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c;
        const double el1 = e[l + 1];
        double s = 0.0, s2 = 0.0;
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < n; ++k) {
            h = V(k, i + 1);
            V(k, i + 1) = s * V(k, i) + c * h;
            V(k, i) = c * V(k, i) - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (fabs(e[l]) > eps * tst1);
    }
    d[l] = d[l] + f;
    e[l] = 0.0;
  }
#undef V
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- dense helpers
bool Cholesky(int n, const double* a, double* l) {
  std::fill(l, l + (size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double d = a[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= l[(size_t)j * n + k] * l[(size_t)j * n + k];
    if (!(d > 0.0)) return false;
    const double ljj = sqrt(d);
    l[(size_t)j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double s = a[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= l[(size_t)i * n + k] * l[(size_t)j * n + k];
      l[(size_t)i * n + j] = s / ljj;
    }
  }
  return true;
}

void InvertLower(int n, const double* l, double* li) {
  std::fill(li, li + (size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    li[(size_t)j * n + j] = 1.0 / l[(size_t)j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= l[(size_t)i * n + k] * li[(size_t)k * n + j];
      li[(size_t)i * n + j] = s / l[(size_t)i * n + i];
    }
  }
}

bool InvertSymmetric(int n, const double* a, double* ai) {
  Mat l((size_t)n * n), li((size_t)n * n);
  if (!Cholesky(n, a, l.data())) return false;
  InvertLower(n, l.data(), li.data());
  // a^-1 = li^T li
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) {
      double s = 0.0;
      for (int k = j; k < n; ++k) s += li[(size_t)k * n + i] * li[(size_t)k * n + j];
      ai[(size_t)i * n + j] = ai[(size_t)j * n + i] = s;
    }
  return true;
}

void SymmetricEig(int n, const double* a, double* s, double* u) {
  if (n < 1) return;
  std::vector<double> v(a, a + (size_t)n * n), d(n), e(n);
  for (int i = 0; i < n; ++i)   // symmetrise (the reduction reads the lower triangle)
    for (int j = 0; j < i; ++j) v[(size_t)i * n + j] = v[(size_t)j * n + i] = 0.5 * (a[(size_t)i * n + j] + a[(size_t)j * n + i]);
  Tred2(n, v.data(), d.data(), e.data());
  Tql2(n, v.data(), d.data(), e.data());
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] > d[y]; });
  for (int c = 0; c < n; ++c) {
    s[c] = d[order[c]];
    for (int r = 0; r < n; ++r) u[(size_t)r * n + c] = v[(size_t)r * n + order[c]];
  }
}

// ---------------------------------------------------------------------------------------------------- estimators
int LdaFromStats(int dim, long n, const double* s_tot, const double* s_bet, const float* mean, double total_covariance_factor,
                 double covariance_floor, int lda_dim, float* out) {
  if (n < 1) throw EngineError("LDA: no vectors");
  if (lda_dim < 1 || lda_dim > dim)
    throw EngineError("LDA dimension " + std::to_string(lda_dim) + " is out of range for input dimension " + std::to_string(dim));
  const size_t dd = (size_t)dim * dim;
  Mat total(dd), within(dd), between(dd), m(dd);
  for (size_t e = 0; e < dd; ++e) {
    total[e] = s_tot[e] / (double)n;
    within[e] = (s_tot[e] - s_bet[e]) / (double)n;
    m[e] = total_covariance_factor * total[e] + (1.0 - total_covariance_factor) * within[e];
    between[e] = total[e] - within[e];
  }
  // normalising transform: tn m tn^T = I
  std::vector<double> s(dim);
  Mat u(dd);
  SymmetricEig(dim, m.data(), s.data(), u.data());
  const double floor = covariance_floor * s[0];
  int floored = 0;
  for (int i = 0; i < dim; ++i)
    if (s[i] < floor) {
      s[i] = floor;
      ++floored;
    }
  Mat tn(dd);
  for (int i = 0; i < dim; ++i) {
    const double f = 1.0 / sqrt(s[i]);
    for (int j = 0; j < dim; ++j) tn[(size_t)i * dim + j] = f * u[(size_t)j * dim + i];
  }
  Mat bp = Sandwich(dim, dim, tn, between);
  std::vector<double> s2(dim);
  Mat u2(dd);
  SymmetricEig(dim, bp.data(), s2.data(), u2.data());
  // L = U2[:, :lda_dim]^T tn, then [L | -L mean] in fp32
  std::vector<float> l((size_t)lda_dim * dim);
  for (int i = 0; i < lda_dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double acc = 0.0;
      for (int k = 0; k < dim; ++k) acc += u2[(size_t)k * dim + i] * tn[(size_t)k * dim + j];
      l[(size_t)i * dim + j] = (float)acc;
    }
  for (int i = 0; i < lda_dim; ++i) {
    double off = 0.0;
    for (int j = 0; j < dim; ++j) {
      out[(size_t)i * (dim + 1) + j] = l[(size_t)i * dim + j];
      off -= (double)l[(size_t)i * dim + j] * (double)mean[j];
    }
    out[(size_t)i * (dim + 1) + dim] = (float)off;
  }
  return floored;
}

int PldaFromStats(int dim, int n_spk, const double* sums, const int32_t* counts, const double* s_tot, const double* s_bet,
                  int num_em_iters, Plda* out, std::vector<std::string>* log) {
  if (n_spk < 1) throw EngineError("PLDA: no speakers");
  const size_t dd = (size_t)dim * dim;
  long n_total = 0;
  for (int k = 0; k < n_spk; ++k) {
    if (counts[k] < 1) throw EngineError("PLDA: a speaker without vectors");
    n_total += counts[k];
  }
  // class means, their sum, the offset scatter; classes in order of their sizes
  Mat means((size_t)n_spk * dim);
  std::vector<double> sum(dim, 0.0);
  for (int k = 0; k < n_spk; ++k)
    for (int d = 0; d < dim; ++d) {
      means[(size_t)k * dim + d] = sums[(size_t)k * dim + d] / counts[k];
      sum[d] += means[(size_t)k * dim + d];
    }
  Mat offset_scatter(dd);
  for (size_t e = 0; e < dd; ++e) offset_scatter[e] = s_tot[e] - s_bet[e];
  std::vector<int> order(n_spk);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] < counts[b]; });

  Mat w = Identity(dim), b = Identity(dim), w_inv(dd), b_inv(dd), mixed(dd), tmp(dd);
  std::vector<double> m(dim), t(dim), wv(dim), mw(dim);
  for (int it = 0; it < num_em_iters; ++it) {
    Mat ws = offset_scatter, bs(dd, 0.0);
    double wc = (double)(n_total - n_spk), bc = 0.0;
    if (!InvertSymmetric(dim, w.data(), w_inv.data()) || !InvertSymmetric(dim, b.data(), b_inv.data()))
      throw EngineError("PLDA: a covariance became singular in iteration " + std::to_string(it));
    int n = -1;
    for (int oi = 0; oi < n_spk; ++oi) {
      const int k = order[oi];
      if (counts[k] != n) {
        n = counts[k];
        for (size_t e = 0; e < dd; ++e) tmp[e] = b_inv[e] + n * w_inv[e];
        if (!InvertSymmetric(dim, tmp.data(), mixed.data())) throw EngineError("PLDA: singular mixed covariance");
      }
      for (int d = 0; d < dim; ++d) m[d] = means[(size_t)k * dim + d] - sum[d] / n_spk;
      for (int i = 0; i < dim; ++i) {
        double s = 0.0;
        for (int j = 0; j < dim; ++j) s += w_inv[(size_t)i * dim + j] * m[j];
        t[i] = n * s;
      }
      for (int i = 0; i < dim; ++i) {
        double s = 0.0;
        for (int j = 0; j < dim; ++j) s += mixed[(size_t)i * dim + j] * t[j];
        wv[i] = s;
        mw[i] = m[i] - s;
      }
      for (int i = 0; i < dim; ++i) {
        double* br = bs.data() + (size_t)i * dim;
        double* wr = ws.data() + (size_t)i * dim;
        const double* mr = mixed.data() + (size_t)i * dim;
        for (int j = 0; j < dim; ++j) {
          br[j] += mr[j] + wv[i] * wv[j];
          wr[j] += n * mr[j] + n * mw[i] * mw[j];
        }
      }
      bc += 1.0;
      wc += 1.0;
    }
    for (size_t e = 0; e < dd; ++e) {
      w[e] = ws[e] / wc;
      b[e] = bs[e] / bc;
    }
    if (log) {
      double tw = 0, tb = 0;
      for (int d = 0; d < dim; ++d) {
        tw += w[(size_t)d * dim + d];
        tb += b[(size_t)d * dim + d];
      }
      std::ostringstream o;
      o << "Plda estimation iteration " << it << " of " << num_em_iters << ": trace of within-class variance " << tw
        << ", of between-class variance " << tb;
      log->push_back(o.str());
    }
  }
  // output: mean, transform = U^T chol(W)^-1, psi = eig(C^-1 B C^-T) floored at zero
  Mat c(dd), ci(dd);
  if (!Cholesky(dim, w.data(), c.data())) throw EngineError("PLDA: within-class covariance is not positive definite");
  InvertLower(dim, c.data(), ci.data());
  Mat bp = Sandwich(dim, dim, ci, b);
  std::vector<double> s(dim);
  Mat u(dd);
  SymmetricEig(dim, bp.data(), s.data(), u.data());
  int floored = 0;
  for (int d = 0; d < dim; ++d)
    if (s[d] < 0.0) {
      s[d] = 0.0;
      ++floored;
    }
  out->dim = dim;
  out->mean.assign(dim, 0.0);
  for (int d = 0; d < dim; ++d) out->mean[d] = sum[d] / n_spk;
  out->transform.assign(dd, 0.0);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double acc = 0.0;
      for (int k = j; k < dim; ++k) acc += u[(size_t)k * dim + i] * ci[(size_t)k * dim + j];   // ci is lower
      out->transform[(size_t)i * dim + j] = acc;
    }
  out->psi = s;
  out->ComputeDerivedVars();
  return floored;
}

namespace {
std::string VecText(const std::vector<double>& v) {   // Kaldi's Vector output: " [ a b c ]"
  std::ostringstream o;
  o << " [ ";
  for (double x : v) o << x << " ";
  o << "]";
  return o.str();
}
}  // namespace

void AdaptPlda(long n, const double* m, const double* v, double mean_diff_scale, double within_covar_scale,
               double between_covar_scale, Plda* plda, double* s_out, std::vector<std::string>* log) {
  if (n < 1) throw EngineError("PLDA adaptation: no vectors");
  const int dim = plda->dim;
  const size_t dd = (size_t)dim * dim;
  for (int d = 0; d < dim; ++d)
    if (!(plda->psi[d] >= 0.0)) throw EngineError("PLDA adaptation: the model's psi must not be negative");
  // the adaptation data's mean and covariance; the covariance also takes mean_diff_scale of the mean shift
  std::vector<double> mu(dim), diff(dim);
  double diff_norm = 0.0;
  for (int d = 0; d < dim; ++d) {
    mu[d] = m[d] / (double)n;
    diff[d] = mu[d] - plda->mean[d];
    diff_norm += diff[d] * diff[d];
  }
  Mat var(dd);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j)
      var[(size_t)i * dim + j] = v[(size_t)i * dim + j] / (double)n - mu[i] * mu[j] + mean_diff_scale * diff[i] * diff[j];
  // T' = diag(1/sqrt(1 + psi)) T: the space where the model's total covariance is I; there T' var T'^T = P diag(s) P^T
  Mat tm(plda->transform);
  for (int i = 0; i < dim; ++i) {
    const double f = 1.0 / sqrt(1.0 + plda->psi[i]);
    for (int j = 0; j < dim; ++j) tm[(size_t)i * dim + j] *= f;
  }
  Mat vp = Sandwich(dim, dim, tm, var);
  std::vector<double> s(dim);
  Mat p(dd);
  SymmetricEig(dim, vp.data(), s.data(), p.data());
  // W = diag(1/(1+psi)), B = diag(psi/(1+psi)) there; seen along P (W2 = P^T W P, B2 = P^T B P), each direction with
  // s_i > 1 gets the scaled excess s_i - 1 on both diagonals
  Mat pt(dd), w(dd, 0.0), b(dd, 0.0);
  for (int i = 0; i < dim; ++i) {
    w[(size_t)i * dim + i] = 1.0 / (1.0 + plda->psi[i]);
    b[(size_t)i * dim + i] = plda->psi[i] / (1.0 + plda->psi[i]);
    for (int j = 0; j < dim; ++j) pt[(size_t)i * dim + j] = p[(size_t)j * dim + i];
  }
  Mat w2 = Sandwich(dim, dim, pt, w), b2 = Sandwich(dim, dim, pt, b);
  for (int i = 0; i < dim; ++i)
    if (s[i] > 1.0) {
      w2[(size_t)i * dim + i] += within_covar_scale * (s[i] - 1.0);
      b2[(size_t)i * dim + i] += between_covar_scale * (s[i] - 1.0);
    }
  // back in the T' space: Wm = P W2 P^T = C C^T, C^-1 Bm C^-T = Q diag(psi') Q^T; the new transform is Q^T C^-1 T'
  Mat wm = Sandwich(dim, dim, p, w2), bm = Sandwich(dim, dim, p, b2);
  Mat c(dd), ci(dd);
  if (!Cholesky(dim, wm.data(), c.data()))
    throw EngineError("PLDA adaptation: the adapted within-class covariance is not positive definite");
  InvertLower(dim, c.data(), ci.data());
  Mat bp = Sandwich(dim, dim, ci, bm);
  std::vector<double> psi(dim);
  Mat q(dd);
  SymmetricEig(dim, bp.data(), psi.data(), q.data());
  Mat cit(dd, 0.0);   // C^-1 T' (C^-1 lower)
  for (int i = 0; i < dim; ++i)
    for (int k = 0; k <= i; ++k) {
      const double x = ci[(size_t)i * dim + k];
      for (int j = 0; j < dim; ++j) cit[(size_t)i * dim + j] += x * tm[(size_t)k * dim + j];
    }
  Mat t(dd, 0.0);
  for (int i = 0; i < dim; ++i)
    for (int k = 0; k < dim; ++k) {
      const double x = q[(size_t)k * dim + i];
      for (int j = 0; j < dim; ++j) t[(size_t)i * dim + j] += x * cit[(size_t)k * dim + j];
    }
  if (log) {
    std::ostringstream o;
    o << "Mean differs from old mean with norm " << sqrt(diff_norm);
    log->push_back(o.str());
    log->push_back("Eigenvalues of adaptation-data total-covariance in space where out-of-domain PLDA total-covariance is unit, are: " +
                   VecText(s));
    log->push_back("Old diagonal of between-class covar was: " + VecText(plda->psi) + ", new diagonal is " + VecText(psi));
  }
  if (s_out) std::copy(s.begin(), s.end(), s_out);
  plda->mean = mu;
  plda->transform = t;
  plda->psi = psi;
  plda->ComputeDerivedVars();
}

// ---------------------------------------------------------------------------------------------------- the model
void Plda::ComputeDerivedVars() {
  offset.assign(dim, 0.0);
  for (int i = 0; i < dim; ++i) {
    double s = 0.0;
    for (int j = 0; j < dim; ++j) s += transform[(size_t)i * dim + j] * mean[j];
    offset[i] = -s;
  }
}

void Plda::SmoothWithinClassCovariance(double s) {
  for (int d = 0; d < dim; ++d) {
    const double c = 1.0 + s * psi[d];
    psi[d] /= c;
    const double f = 1.0 / sqrt(c);
    for (int j = 0; j < dim; ++j) transform[(size_t)d * dim + j] *= f;
  }
  ComputeDerivedVars();
}

void ReadPlda(const std::string& rxfilename, Plda* p) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ExpectToken(in, binary, "<Plda>");
  int rows = 0, cols = 0;
  ReadVectorDouble(in, binary, &p->mean);
  ReadMatrixDouble(in, binary, &rows, &cols, &p->transform);
  ReadVectorDouble(in, binary, &p->psi);
  ExpectToken(in, binary, "</Plda>");
  const int st = in.Close();
  if (st != 0) throw KioError("reading the PLDA model from " + rxfilename + ": the command exited with status " + std::to_string(st));
  p->dim = (int)p->mean.size();
  if (p->dim < 1 || rows != p->dim || cols != p->dim || (int)p->psi.size() != p->dim)
    throw KioError("inconsistent PLDA model in " + rxfilename + ": mean " + std::to_string(p->mean.size()) + ", transform " +
                   std::to_string(rows) + " x " + std::to_string(cols) + ", psi " + std::to_string(p->psi.size()));
  p->ComputeDerivedVars();
}

void WritePlda(const std::string& wxfilename, bool binary, const Plda& p) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteToken(out, binary, "<Plda>");
  WriteVectorDouble(out, binary, p.mean.data(), p.dim);
  WriteMatrixDouble(out, binary, p.transform.data(), p.dim, p.dim);
  WriteVectorDouble(out, binary, p.psi.data(), p.dim);
  WriteToken(out, binary, "</Plda>");
  if (!binary) out.Put('\n');
  out.Close();
}

// ---------------------------------------------------------------------------------------------------- device entry points
void ScatterStats(int device, const float* x, int n, int dim, const int32_t* seg_off, const int32_t* idx, int n_seg,
                  double* s_tot, double* sums, double* s_bet, float* device_ms) {
  if (n < 0 || dim < 1 || n_seg < 0) throw EngineError("ScatterStats: bad shape");
  if (seg_off[0] != 0) throw EngineError("ScatterStats: segment offsets must start at 0");
  for (int s = 0; s < n_seg; ++s)
    if (seg_off[s + 1] < seg_off[s]) throw EngineError("ScatterStats: segment offsets must not decrease");
  const int n_idx = seg_off[n_seg];
  for (int i = 0; i < n_idx; ++i)
    if (idx[i] < 0 || idx[i] >= n) throw EngineError("ScatterStats: row index out of range");
  UseDevice(device, kWhoNeeds);
  const size_t dd = (size_t)dim * dim;
  DevBuf dx((size_t)n * dim * 4), doff((size_t)(n_seg + 1) * 4), didx((size_t)n_idx * 4), dsums((size_t)n_seg * dim * 8);
  DevBuf dtot(dd * 8), dbet(dd * 8), dwork(scatter_stats_workspace(dim, n_idx, n_seg) * 8);
  dx.Upload(x, (size_t)n * dim * 4, "copy vectors");
  doff.Upload(seg_off, (size_t)(n_seg + 1) * 4, "copy segment offsets");
  didx.Upload(idx, (size_t)n_idx * 4, "copy row indices");
  ScatterArgs a;
  a.x = dx.as<float>();
  a.dim = dim;
  a.ldx = dim;
  a.seg_off = doff.as<int32_t>();
  a.idx = didx.as<int32_t>();
  a.n_seg = n_seg;
  a.n_idx = n_idx;
  a.sums = dsums.as<double>();
  a.s_tot = dtot.as<double>();
  a.s_bet = dbet.as<double>();
  a.work = dwork.as<double>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_scatter_stats(a, nullptr), "scatter statistics kernel launch");
  if (device_ms) *device_ms = tm.Stop();
  if (s_tot) dtot.Download(s_tot, dd * 8, "copy total scatter");
  if (s_bet) dbet.Download(s_bet, dd * 8, "copy between-class scatter");
  if (sums) dsums.Download(sums, (size_t)n_seg * dim * 8, "copy speaker sums");
}

void PldaTransform(int device, const float* x, int n, int dim, const double* transform, const double* offset,
                   const double* psi, const double* num, bool normalize, bool simple, float* y, double* scale,
                   float* device_ms) {
  if (n < 0 || dim < 1) throw EngineError("PldaTransform: bad shape");
  if (dim > kPldaMaxDim)
    throw EngineError("PLDA dimension " + std::to_string(dim) + " is larger than the device kernels support (" +
                      std::to_string(kPldaMaxDim) + ")");
  for (int i = 0; i < n; ++i)
    if (!(num[i] > 0)) throw EngineError("PldaTransform: example counts must be positive");
  UseDevice(device, kWhoNeeds);
  if (n == 0) return;
  const size_t dd = (size_t)dim * dim;
  std::vector<double> tt(dd);
  for (int d = 0; d < dim; ++d)
    for (int k = 0; k < dim; ++k) tt[(size_t)k * dim + d] = transform[(size_t)d * dim + k];
  DevBuf dx((size_t)n * dim * 4), dt(dd * 8), doff((size_t)dim * 8), dpsi((size_t)dim * 8), dnum((size_t)n * 8);
  DevBuf dy((size_t)n * dim * 4), dscale((size_t)n * 8);
  dx.Upload(x, (size_t)n * dim * 4, "copy vectors");
  dt.Upload(tt.data(), dd * 8, "copy transform");
  doff.Upload(offset, (size_t)dim * 8, "copy offset");
  dpsi.Upload(psi, (size_t)dim * 8, "copy psi");
  dnum.Upload(num, (size_t)n * 8, "copy counts");
  PldaTransformArgs a;
  a.x = dx.as<float>();
  a.n = n;
  a.dim = dim;
  a.tt = dt.as<double>();
  a.offset = doff.as<double>();
  a.psi = dpsi.as<double>();
  a.num = dnum.as<double>();
  a.normalize = normalize ? 1 : 0;
  a.simple = simple ? 1 : 0;
  a.y = dy.as<float>();
  a.scale = dscale.as<double>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_plda_transform(a, nullptr), "PLDA transform kernel launch");
  if (device_ms) *device_ms = tm.Stop();
  dy.Download(y, (size_t)n * dim * 4, "copy transformed vectors");
  if (scale) dscale.Download(scale, (size_t)n * 8, "copy scales");
}

void PldaScore(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim,
               const double* psi, const int32_t* trials, long n_trials, double* scores, float* device_ms) {
  if (n_u < 0 || n_v < 0 || dim < 1 || n_trials < 0) throw EngineError("PldaScore: bad shape");
  if (dim > kPldaMaxDim)
    throw EngineError("PLDA dimension " + std::to_string(dim) + " is larger than the device kernels support (" +
                      std::to_string(kPldaMaxDim) + ")");
  for (long i = 0; i < n_trials; ++i)
    if (trials[2 * i] < 0 || trials[2 * i] >= n_u || trials[2 * i + 1] < 0 || trials[2 * i + 1] >= n_v)
      throw EngineError("PldaScore: trial " + std::to_string(i) + " indexes a row that does not exist");
  for (int k = 0; k < n_u; ++k)
    if (!(num_u[k] > 0)) throw EngineError("PldaScore: example counts must be positive");
  UseDevice(device, kWhoNeeds);
  if (n_trials == 0) return;
  std::vector<double> inv_psi1(dim);
  for (int d = 0; d < dim; ++d) inv_psi1[d] = 1.0 / (1.0 + psi[d]);
  DevBuf du((size_t)n_u * dim * 4), dnum((size_t)n_u * 8), dv((size_t)n_v * dim * 4), dpsi((size_t)dim * 8);
  DevBuf dip((size_t)dim * 8), dtr((size_t)n_trials * 8), dwork((size_t)n_u * (2 * dim + 1) * 8), dsc((size_t)n_trials * 8);
  du.Upload(u, (size_t)n_u * dim * 4, "copy enrolment vectors");
  dnum.Upload(num_u, (size_t)n_u * 8, "copy counts");
  dv.Upload(v, (size_t)n_v * dim * 4, "copy test vectors");
  dpsi.Upload(psi, (size_t)dim * 8, "copy psi");
  dip.Upload(inv_psi1.data(), (size_t)dim * 8, "copy psi");
  dtr.Upload(trials, (size_t)n_trials * 8, "copy trials");
  PldaScoreArgs a;
  a.u = du.as<float>();
  a.num_u = dnum.as<double>();
  a.n_u = n_u;
  a.v = dv.as<float>();
  a.n_v = n_v;
  a.dim = dim;
  a.psi = dpsi.as<double>();
  a.inv_psi1 = dip.as<double>();
  a.trials = dtr.as<int32_t>();
  a.n_trials = n_trials;
  a.work = dwork.as<double>();
  a.scores = dsc.as<double>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_plda_score(a, nullptr), "PLDA scoring kernel launch");
  if (device_ms) *device_ms = tm.Stop();
  dsc.Download(scores, (size_t)n_trials * 8, "copy scores");
}

}  // namespace xv
