// i-vector extraction: what ivector-extract does in sid/extract_ivectors.sh:69.  [UPSTREAM, recalled]: a restatement of Kaldi's
// ivector/ivector-extractor.cc and ivectorbin/ivector-extract.cc of early 2018, written from their documented behaviour; Kaldi is
// not part of the reference tree, so parity with a Kaldi binary is not pinned by any test here.  tests/ivector_ref.py is the same
// in numpy.
//
// Model file (final.ie), binary or text:
//   <IvectorExtractor> <w> DM <w_vec> DV <M> int32 G, G x DM (each D x S) <SigmaInv> G x (DP: packed lower triangle, D (D + 1) / 2)
//   <IvectorOffset> double </IvectorExtractor>
//   A model whose <w> has rows has i-vector-dependent weights; no recipe trains one and it is refused by name.
// Derived once per model, fp64:
//   SigmaInvM_g = Sigma_g^-1 M_g (D x S);  U_g = the packed lower triangle of M_g' Sigma_g^-1 M_g, P = S (S + 1) / 2 values, the
//   index of (r, c), r >= c, being r (r + 1) / 2 + c.
// Per utterance, from features x_t (fp32) and posteriors (g, w) (fp32), with p the prior offset:
//   1. tot = acoustic_weight * float(sum of w in fp64, frame order).  max_count > 0 and tot > max_count: every posterior is
//      multiplied by float(acoustic_weight * max_count / tot) (and the tool logs it); otherwise by float(acoustic_weight).  The
//      multiplication is fp32.  The defaults (1.0, 0) change nothing.
//   2. gamma_g = sum_t w, X_g = sum_t w x_t: fp64, frames ascending.  double(w) * double(x) is exact (24 + 24 bits), so the
//      statistics are one fixed set of bits with or without a fused multiply-add.
//   3. l = sum_g SigmaInvM_g' X_g;  l_0 += p.
//   4. Q = unpack(sum_g gamma_g U_g) + I.
//   5. Q x = l by Cholesky.  A factorisation that fails is an error of that utterance.
//   6. the change of the auxiliary function: F(x) - F(p e_0), F(v) = l . v - v' Q v / 2, from the unfactored Q (everything else in
//      Kaldi's auxiliary function is constant in v).
//   7. the output is float(x) with p taken off element 0 before the rounding.
//
// On the device (ivex_kernels.h) everything is fp64 with summation orders that are functions of the utterance and the model alone.
// Limits: i-vector dimension S <= 1024, feature dimension D <= 96; no limit on the number of Gaussians beyond memory.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kio.h"

namespace xv {

struct IvexData {
  int G = 0, D = 0, S = 0;
  std::vector<double> w_vec;       // [G]
  std::vector<double> M;           // [G][D][S]
  std::vector<double> sigma_inv;   // [G][D (D + 1) / 2]
  double prior_offset = 0.0;
};
// Host only.  rxfilename / wxfilename: "file", "-", "cmd |".  KioError: a truncated or malformed file, a model with <w> rows.
void ReadIvexFile(const std::string& rxfilename, IvexData* m);
void WriteIvexFile(const std::string& wxfilename, bool binary, const IvexData& m);

// Host only: the fp32 scale step 1 gives an utterance's posteriors; *clipped: the max-count rule was the one that applied.
float IvexPosteriorScale(const float* w, size_t n, double acoustic_weight, double max_count, bool* clipped, double* tot = nullptr);

// A model on one device: the derived variables are computed there at creation, the workspaces allocated once.
class IvexModel {
 public:
  ~IvexModel();
  int device() const;
  int num_gauss() const;
  int feat_dim() const;
  int ivector_dim() const;
  float derive_ms() const;
  double prior_offset() const;
  const std::vector<double>& w_vec() const;       // host copies of the two small arrays of the model
  const std::vector<double>& sigma_inv() const;
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
IvexModel* IvexCreate(int device, const IvexData& m);
// sigma_inv_m [G D][S], U [G][S (S + 1) / 2]; either may be null
void IvexDerived(const IvexModel& m, double* sigma_inv_m, double* U);

struct IvexOutputs {
  float* ivectors = nullptr;      // [n][S]
  int32_t* status = nullptr;      // [n]: 0, or 1 where Q was not positive definite (that row of ivectors is zero)
  // each may be null
  double* auxf_change = nullptr;  // [n]
  double* gamma = nullptr;        // [n][G]
  double* X = nullptr;            // [n][G D]
  double* linear = nullptr;       // [n][S]
  double* quadratic = nullptr;    // [n][S (S + 1) / 2], the packed lower triangle of Q
  float* device_ms4 = nullptr;    // {statistics, quadratic GEMM, linear GEMM, solve}, added up over the launch groups
};
// feats [row_off[n_utts]][D]; frame t has the pairs post_off[t] .. post_off[t + 1] of (post_idx, post_w).  Blocking.  KioError: a
// Gaussian index outside the model (checked before anything is uploaded).
// after_group (may be null; out.status is required with or without it, and is what the hook's status points into) is called once
// per launch group, after the group's status came back and before the next group's
// launches: the E-step of training (ivex_train.h) reads the group's device results there.
struct IvexGroupView {
  int u0, B;                // the group is the utterances u0 .. u0 + B of the call
  const int32_t* status;    // host, [B]
  // device, per utterance of the group
  const double* gamma;      // [B][G]
  const double* X;          // [B][G D]
  const double* linear;     // [B][S]
  const double* quadratic;  // [B][S (S + 1) / 2] packed Q
  const double* work;       // [B][S + 1][S]: the Cholesky factor of Q in the lower triangle
  const double* solution;   // [B][S] the fp64 solution, with the prior offset
};
typedef std::function<void(const IvexGroupView&)> IvexGroupHook;
void IvexExtract(IvexModel& m, const float* feats, const int32_t* row_off, int n_utts, const int32_t* post_off, const int32_t* post_idx,
                 const float* post_w, double acoustic_weight, double max_count, const IvexOutputs& out, const IvexGroupHook* after_group = nullptr);

}  // namespace xv
