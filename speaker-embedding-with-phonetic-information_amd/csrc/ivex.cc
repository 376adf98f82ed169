#include "ivex.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "bucket_sort.h"
#include "device.h"
#include "ivex_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "i-vector extraction needs";
static_assert(kIvexMaxBatch <= kBucketSortMaxSegments, "a launch group's utterances are the segments of one sort");

// DP / FP (binary) or " [ rows ]" (text): one packed lower triangle appended to *packed; returns its dimension
int ReadPackedDouble(Input& in, bool binary, std::vector<double>* packed) {
  std::vector<double> v;
  int dim = 0;
  if (binary) {
    std::string tok;
    ReadToken(in, true, &tok);
    if (tok != "FP" && tok != "DP") throw KioError("expected token FP or DP, got " + tok);
    dim = ReadInt32(in, true);
    if (dim < 0 || dim > 65535) throw KioError("bad packed-matrix dimension " + std::to_string(dim));
    const size_t n = (size_t)dim * (dim + 1) / 2;
    if (tok == "DP") {
      v.resize(n);
      if (n) in.Read(v.data(), n * 8);
    } else {
      std::vector<float> f(n);
      if (n) in.Read(f.data(), n * 4);
      v.assign(f.begin(), f.end());
    }
  } else {
    ReadVectorDouble(in, false, &v);
    while ((size_t)dim * (dim + 1) / 2 < v.size()) ++dim;
    if ((size_t)dim * (dim + 1) / 2 != v.size()) throw KioError("a text packed matrix with " + std::to_string(v.size()) + " values is no triangle");
  }
  packed->insert(packed->end(), v.begin(), v.end());
  return dim;
}

void WritePackedDouble(Output& out, bool binary, const double* p, int dim) {
  if (binary) {
    out.Puts("DP ");
    WriteInt32(out, true, dim);
    out.Write(p, (size_t)dim * (dim + 1) / 2 * 8);
    return;
  }
  if (dim == 0) {
    out.Puts(" [ ]\n");
    return;
  }
  out.Puts(" [\n");
  char buf[48];
  for (int i = 0; i < dim; ++i) {
    out.Puts("  ");
    for (int j = 0; j <= i; ++j) {
      snprintf(buf, sizeof buf, "%.17g ", *p++);
      out.Puts(buf);
    }
    out.Puts(i + 1 == dim ? "]\n" : "\n");
  }
}

void CheckShape(const IvexData& m) {
  if (m.G < 1 || m.D < 1 || m.S < 1) throw KioError("i-vector extractor: a model needs at least one Gaussian, one feature and one i-vector dimension");
  if (m.S > kIvexMaxS)
    throw KioError("the i-vector dimension " + std::to_string(m.S) + " is above the device solve's limit of " + std::to_string(kIvexMaxS));
  if (m.D > kIvexMaxDim)
    throw KioError("the model's feature dimension " + std::to_string(m.D) + " is above the device kernels' limit of " + std::to_string(kIvexMaxDim));
  const size_t tri = (size_t)m.D * (m.D + 1) / 2;
  if (m.M.size() != (size_t)m.G * m.D * m.S || m.sigma_inv.size() != (size_t)m.G * tri || m.w_vec.size() != (size_t)m.G)
    throw KioError("i-vector extractor: the arrays do not have the model's shape");
}

}  // namespace

void ReadIvexFile(const std::string& rxfilename, IvexData* m) {
  *m = IvexData();
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ExpectToken(in, binary, "<IvectorExtractor>");
  ExpectToken(in, binary, "<w>");
  int wr = 0, wc = 0;
  std::vector<double> w;
  ReadMatrixDouble(in, binary, &wr, &wc, &w);
  if (wr != 0)
    throw KioError("the model " + rxfilename + " has i-vector-dependent weights (a <w> matrix with " + std::to_string(wr) +
                   " rows): that path is not built, no recipe trains such a model (use_weights=false)");
  ExpectToken(in, binary, "<w_vec>");
  ReadVectorDouble(in, binary, &m->w_vec);
  ExpectToken(in, binary, "<M>");
  const int32_t G = ReadInt32(in, binary);
  if (G < 1 || G > (1 << 24)) throw KioError("bad number of Gaussians " + std::to_string(G) + " in " + rxfilename);
  if (m->w_vec.size() != (size_t)G) throw KioError("<w_vec> has " + std::to_string(m->w_vec.size()) + " entries, <M> " + std::to_string(G) + " matrices");
  m->G = G;
  std::vector<double> one;
  for (int g = 0; g < G; ++g) {
    int r = 0, c = 0;
    ReadMatrixDouble(in, binary, &r, &c, &one);
    if (g == 0) {
      m->D = r;
      m->S = c;
      if (r < 1 || c < 1) throw KioError("an empty projection matrix in " + rxfilename);
    } else if (r != m->D || c != m->S) {
      throw KioError("projection matrix " + std::to_string(g) + " is " + std::to_string(r) + " x " + std::to_string(c) + ", the first one " +
                     std::to_string(m->D) + " x " + std::to_string(m->S));
    }
    m->M.insert(m->M.end(), one.begin(), one.end());
  }
  ExpectToken(in, binary, "<SigmaInv>");
  for (int g = 0; g < G; ++g) {
    const int dim = ReadPackedDouble(in, binary, &m->sigma_inv);
    if (dim != m->D) throw KioError("inverse covariance " + std::to_string(g) + " has dimension " + std::to_string(dim) + ", the projections " + std::to_string(m->D));
  }
  ExpectToken(in, binary, "<IvectorOffset>");
  m->prior_offset = ReadFloatOrDouble(in, binary);
  ExpectToken(in, binary, "</IvectorExtractor>");
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
}

void WriteIvexFile(const std::string& wxfilename, bool binary, const IvexData& m) {
  const size_t tri = (size_t)m.D * (m.D + 1) / 2;
  if (m.G < 1 || m.D < 1 || m.S < 1 || m.M.size() != (size_t)m.G * m.D * m.S || m.sigma_inv.size() != (size_t)m.G * tri || m.w_vec.size() != (size_t)m.G)
    throw KioError("i-vector extractor: the arrays do not have the model's shape");
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteToken(out, binary, "<IvectorExtractor>");
  WriteToken(out, binary, "<w>");
  WriteMatrixDouble(out, binary, nullptr, 0, 0);
  WriteToken(out, binary, "<w_vec>");
  WriteVectorDouble(out, binary, m.w_vec.data(), m.G);
  WriteToken(out, binary, "<M>");
  WriteInt32(out, binary, m.G);
  for (int g = 0; g < m.G; ++g) WriteMatrixDouble(out, binary, m.M.data() + (size_t)g * m.D * m.S, m.D, m.S);
  WriteToken(out, binary, "<SigmaInv>");
  for (int g = 0; g < m.G; ++g) WritePackedDouble(out, binary, m.sigma_inv.data() + (size_t)g * tri, m.D);
  WriteToken(out, binary, "<IvectorOffset>");
  WriteDouble(out, binary, m.prior_offset);
  WriteToken(out, binary, "</IvectorExtractor>");
  if (!binary) out.Put('\n');
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

float IvexPosteriorScale(const float* w, size_t n, double acoustic_weight, double max_count, bool* clipped, double* tot_out) {
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i) sum += (double)w[i];
  const double tot = acoustic_weight * (double)(float)sum;
  if (tot_out) *tot_out = tot;
  const bool clip = max_count > 0.0 && tot > max_count;
  if (clipped) *clipped = clip;
  return clip ? (float)(acoustic_weight * max_count / tot) : (float)acoustic_weight;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct IvexModel::Impl {
  int device = 0, G = 0, D = 0, S = 0, lin_chunks = 0;
  int64_t P = 0;
  double prior_offset = 0.0;
  float derive_ms = 0.f;
  std::vector<double> w_vec, sigma_inv;   // host
  DevBuf sigma_inv_m, U;
  DevBuf solution;                        // [B][S] fp64, allocated by the first call that has a group hook
  // workspaces of one launch group, allocated once
  DevBuf gamma, X, partial, linear, quadratic, work, ivec, auxf, status;
  // what follows the group's frames and pairs: grown when a group needs more
  DevBuf feats, pair_frame, pair_gauss, pair_w;
  BucketSorter sort;   // one segment per utterance of the group
};

IvexModel::~IvexModel() {}
int IvexModel::device() const { return impl_->device; }
int IvexModel::num_gauss() const { return impl_->G; }
int IvexModel::feat_dim() const { return impl_->D; }
int IvexModel::ivector_dim() const { return impl_->S; }
float IvexModel::derive_ms() const { return impl_->derive_ms; }
double IvexModel::prior_offset() const { return impl_->prior_offset; }
const std::vector<double>& IvexModel::w_vec() const { return impl_->w_vec; }
const std::vector<double>& IvexModel::sigma_inv() const { return impl_->sigma_inv; }

IvexModel* IvexCreate(int device, const IvexData& m) {
  CheckShape(m);
  UseDevice(device, kWhoNeeds);
  std::unique_ptr<IvexModel> h(new IvexModel);
  h->impl_.reset(new IvexModel::Impl);
  IvexModel::Impl& I = *h->impl_;
  I.device = device;
  I.G = m.G;
  I.D = m.D;
  I.S = m.S;
  I.P = (int64_t)m.S * (m.S + 1) / 2;
  I.prior_offset = m.prior_offset;
  I.w_vec = m.w_vec;
  I.sigma_inv = m.sigma_inv;
  const int64_t K = (int64_t)m.G * m.D;
  I.lin_chunks = (int)((K + kIvexKChunk - 1) / kIvexKChunk);
  I.sigma_inv_m.Reserve((size_t)K * m.S * 8);
  I.U.Reserve((size_t)m.G * I.P * 8);
  {
    DevBuf d_m, d_sig;
    d_m.Upload(m.M, "copy the projections");
    d_sig.Upload(m.sigma_inv, "copy the inverse covariances");
    IvexDeriveArgs a;
    memset(&a, 0, sizeof a);
    a.M = d_m.as<double>();
    a.sigma_inv = d_sig.as<double>();
    a.G = m.G;
    a.D = m.D;
    a.S = m.S;
    a.sigma_inv_m = I.sigma_inv_m.as<double>();
    a.U = I.U.as<double>();
    EventTimer tm(true);
    tm.Start();
    Check(launch_ivex_derive(a, nullptr), "ivex_derive launch");
    I.derive_ms = tm.Stop();
    Check(hipDeviceSynchronize(), "ivex_derive");
  }
  const size_t B = kIvexMaxBatch;
  I.gamma.Reserve(B * m.G * 8);
  I.X.Reserve(B * (size_t)K * 8);
  I.partial.Reserve((size_t)I.lin_chunks * B * m.S * 8);
  I.linear.Reserve(B * m.S * 8);
  I.quadratic.Reserve(B * (size_t)I.P * 8);
  I.work.Reserve(B * (size_t)(m.S + 1) * m.S * 8);
  I.ivec.Reserve(B * m.S * 4);
  I.auxf.Reserve(B * 8);
  I.status.Reserve(B * 4);
  return h.release();
}

void IvexDerived(const IvexModel& m, double* sigma_inv_m, double* U) {
  const IvexModel::Impl& I = *m.impl_;
  UseDevice(I.device, kWhoNeeds);
  if (sigma_inv_m) Check(hipMemcpy(sigma_inv_m, I.sigma_inv_m.p, (size_t)I.G * I.D * I.S * 8, hipMemcpyDeviceToHost), "copy SigmaInvM");
  if (U) Check(hipMemcpy(U, I.U.p, (size_t)I.G * I.P * 8, hipMemcpyDeviceToHost), "copy U");
}

void IvexExtract(IvexModel& m, const float* feats, const int32_t* row_off, int n_utts, const int32_t* post_off, const int32_t* post_idx,
                 const float* post_w, double acoustic_weight, double max_count, const IvexOutputs& out, const IvexGroupHook* after_group) {
  IvexModel::Impl& I = *m.impl_;
  if (out.device_ms4) out.device_ms4[0] = out.device_ms4[1] = out.device_ms4[2] = out.device_ms4[3] = 0.f;
  if (n_utts < 0 || !row_off || row_off[0] != 0) throw KioError("ivector-extract: bad argument");
  for (int u = 0; u < n_utts; ++u)
    if (row_off[u + 1] < row_off[u]) throw KioError("ivector-extract: row offsets must not decrease");
  if (n_utts == 0) return;
  const int64_t rows = row_off[n_utts];
  if (!out.ivectors || !out.status || !post_off || (rows && !feats)) throw KioError("ivector-extract: null buffer");
  if (post_off[0] != 0) throw KioError("ivector-extract: posterior offsets must start at 0");
  for (int64_t t = 0; t < rows; ++t)
    if (post_off[t + 1] < post_off[t]) throw KioError("ivector-extract: posterior offsets must not decrease");
  const int64_t pairs_all = post_off[rows];
  if (pairs_all && (!post_idx || !post_w)) throw KioError("ivector-extract: null buffer");
  for (int64_t i = 0; i < pairs_all; ++i)
    if (post_idx[i] < 0 || post_idx[i] >= I.G)
      throw KioError("ivector-extract: the posteriors name Gaussian " + std::to_string(post_idx[i]) + "; the model has " + std::to_string(I.G));
  UseDevice(I.device, kWhoNeeds);
  if (after_group) I.solution.Reserve((size_t)kIvexMaxBatch * I.S * 8);
  constexpr int64_t kBatchFrames = 1 << 16;
  const int G = I.G, D = I.D, S = I.S;
  const int64_t K = (int64_t)G * D;
  std::vector<int32_t> pair_frame, pair_gauss, pair_off;
  std::vector<float> pair_w;
  for (int u0 = 0; u0 < n_utts;) {
    int u1 = u0 + 1;
    while (u1 < n_utts && u1 - u0 < kIvexMaxBatch && row_off[u1 + 1] - row_off[u0] <= kBatchFrames) ++u1;
    const int B = u1 - u0;
    const int64_t r0 = row_off[u0], nr = row_off[u1] - r0;
    // the group's pairs, scaled (step 1); pair_off: the utterances are the segments of the sort
    pair_frame.clear();
    pair_gauss.clear();
    pair_w.clear();
    pair_off.assign(1, 0);
    for (int u = u0; u < u1; ++u) {
      const int64_t pa = post_off[row_off[u]], pb = post_off[row_off[u + 1]];
      const float scale = IvexPosteriorScale(post_w + pa, (size_t)(pb - pa), acoustic_weight, max_count, nullptr);
      for (int64_t t = row_off[u]; t < row_off[u + 1]; ++t)
        for (int64_t i = post_off[t]; i < post_off[t + 1]; ++i) {
          pair_frame.push_back((int32_t)(t - r0));
          pair_gauss.push_back(post_idx[i]);
          pair_w.push_back(post_w[i] * scale);
        }
      pair_off.push_back((int32_t)pair_frame.size());
    }
    const size_t pairs = pair_frame.size();
    I.feats.Upload(feats + (size_t)r0 * D, (size_t)nr * D * 4, "copy features");
    I.pair_frame.Upload(pair_frame, "copy the posteriors");
    I.pair_gauss.Upload(pair_gauss, "copy the posteriors");
    I.pair_w.Upload(pair_w, "copy the posteriors");

    IvexStatsArgs st;
    memset(&st, 0, sizeof st);
    st.feats = I.feats.as<float>();
    st.D = D;
    st.G = G;
    st.B = B;
    st.pair_frame = I.pair_frame.as<int32_t>();
    st.pair_gauss = I.pair_gauss.as<int32_t>();
    st.pair_w = I.pair_w.as<float>();
    st.gamma = I.gamma.as<double>();
    st.X = I.X.as<double>();
    IvexGemmArgs quad;
    memset(&quad, 0, sizeof quad);
    quad.A = I.gamma.as<double>();
    quad.W = I.U.as<double>();
    quad.B = B;
    quad.K = G;
    quad.N = I.P;
    quad.k_chunk = G;   // thousands of column tiles: K is not split
    quad.C = I.quadratic.as<double>();
    IvexGemmArgs lin;
    memset(&lin, 0, sizeof lin);
    lin.A = I.X.as<double>();
    lin.W = I.sigma_inv_m.as<double>();
    lin.B = B;
    lin.K = K;
    lin.N = S;
    lin.k_chunk = kIvexKChunk;
    lin.C = I.partial.as<double>();
    IvexFinishArgs fin;
    memset(&fin, 0, sizeof fin);
    fin.partial = I.partial.as<double>();
    fin.chunks = I.lin_chunks;
    fin.B = B;
    fin.S = S;
    fin.prior_offset = I.prior_offset;
    fin.linear = I.linear.as<double>();
    fin.quadratic = I.quadratic.as<double>();
    IvexSolveArgs so;
    memset(&so, 0, sizeof so);
    so.quadratic = I.quadratic.as<double>();
    so.linear = I.linear.as<double>();
    so.B = B;
    so.S = S;
    so.prior_offset = I.prior_offset;
    so.work = I.work.as<double>();
    so.ivector = I.ivec.as<float>();
    so.auxf_change = out.auxf_change ? I.auxf.as<double>() : nullptr;
    so.status = I.status.as<int32_t>();
    so.solution = after_group ? I.solution.as<double>() : nullptr;

    EventTimer tm(out.device_ms4 != nullptr, 5);
    tm.Mark();
    Check(I.sort.Run(st.pair_gauss, (int64_t)pairs, pair_off.data(), B, G, nullptr), "bucket_sort launch");
    st.bucket_start = I.sort.start.as<int32_t>();   // Run sizes them
    st.sorted = I.sort.sorted.as<int32_t>();
    Check(launch_ivex_stats(st, nullptr), "ivex_stats launch");
    tm.Mark();
    Check(launch_ivex_gemm(quad, nullptr), "ivex_gemm launch (quadratic term)");
    tm.Mark();
    Check(launch_ivex_gemm(lin, nullptr), "ivex_gemm launch (linear term)");
    Check(launch_ivex_finish_terms(fin, nullptr), "ivex_finish_terms launch");
    tm.Mark();
    Check(launch_ivex_solve(so, nullptr), "ivex_solve launch");
    tm.Mark();
    if (out.device_ms4)
      for (int i = 0; i < 4; ++i) out.device_ms4[i] += tm.Span(i);
    Check(hipMemcpy(out.ivectors + (size_t)u0 * S, I.ivec.p, (size_t)B * S * 4, hipMemcpyDeviceToHost), "copy the i-vectors");
    Check(hipMemcpy(out.status + u0, I.status.p, (size_t)B * 4, hipMemcpyDeviceToHost), "copy the status");
    if (out.auxf_change) Check(hipMemcpy(out.auxf_change + u0, I.auxf.p, (size_t)B * 8, hipMemcpyDeviceToHost), "copy the objective changes");
    if (out.gamma) Check(hipMemcpy(out.gamma + (size_t)u0 * G, I.gamma.p, (size_t)B * G * 8, hipMemcpyDeviceToHost), "copy gamma");
    if (out.X) Check(hipMemcpy(out.X + (size_t)u0 * K, I.X.p, (size_t)B * K * 8, hipMemcpyDeviceToHost), "copy X");
    if (out.linear) Check(hipMemcpy(out.linear + (size_t)u0 * S, I.linear.p, (size_t)B * S * 8, hipMemcpyDeviceToHost), "copy the linear term");
    if (out.quadratic)
      Check(hipMemcpy(out.quadratic + (size_t)u0 * I.P, I.quadratic.p, (size_t)B * I.P * 8, hipMemcpyDeviceToHost), "copy the quadratic term");
    if (after_group) {
      IvexGroupView v;
      v.u0 = u0;
      v.B = B;
      v.status = out.status + u0;
      v.gamma = I.gamma.as<double>();
      v.X = I.X.as<double>();
      v.linear = I.linear.as<double>();
      v.quadratic = I.quadratic.as<double>();
      v.work = I.work.as<double>();
      v.solution = I.solution.as<double>();
      (*after_group)(v);
    }
    u0 = u1;
  }
}

}  // namespace xv
