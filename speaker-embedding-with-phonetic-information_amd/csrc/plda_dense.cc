// Host side of adaptive score normalisation (plda.h): the plan that cuts a score matrix into row chunks of a bounded device
// workspace, and the driver that produces each chunk with the dense scoring kernel and hands it to a consumer - the top-N
// statistics kernel, or a copy to the host.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "device.h"
#include "plda.h"
#include "plda_dense_kernels.h"

namespace xv {
namespace {

const char kWhoNeeds[] = "the PLDA back-end kernels need";

void CheckDim(int dim) {
  if (dim > kPldaMaxDim)
    throw EngineError("PLDA dimension " + std::to_string(dim) + " is larger than the device kernels support (" +
                      std::to_string(kPldaMaxDim) + ")");
}

// What one call works on: both prepared operands on the device, and which of them gives the rows of the score matrix.
struct DenseOperands {
  DevBuf a, r, b;   // [n_u][ks] and [n_u] of the enrolment table, [n_v][ks] of the test table
  int n_u = 0, n_v = 0, ks = 0;
  bool rows_are_v = false;
  int64_t rows() const { return rows_are_v ? n_v : n_u; }
  int cols() const { return rows_are_v ? n_u : n_v; }
};

void Prepare(const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim, const double* psi, bool rows_are_v,
             DenseOperands* o) {
  std::vector<double> inv_psi1(dim);
  for (int d = 0; d < dim; ++d) inv_psi1[d] = 1.0 / (1.0 + psi[d]);
  DevBuf du((size_t)n_u * dim * 4), dnum((size_t)n_u * 8), dv((size_t)n_v * dim * 4), dpsi((size_t)dim * 8), dip((size_t)dim * 8);
  du.Upload(u, (size_t)n_u * dim * 4, "copy enrolment vectors");
  dnum.Upload(num_u, (size_t)n_u * 8, "copy counts");
  dv.Upload(v, (size_t)n_v * dim * 4, "copy test vectors");
  dpsi.Upload(psi, (size_t)dim * 8, "copy psi");
  dip.Upload(inv_psi1.data(), (size_t)dim * 8, "copy psi");
  o->n_u = n_u;
  o->n_v = n_v;
  o->ks = dense_k_stride(dim);
  o->rows_are_v = rows_are_v;
  o->a.Alloc((size_t)n_u * o->ks * 8);
  o->r.Alloc((size_t)n_u * 8);
  o->b.Alloc((size_t)n_v * o->ks * 8);
  DensePrepArgs p;
  p.u = du.as<float>();
  p.num_u = dnum.as<double>();
  p.n_u = n_u;
  p.v = dv.as<float>();
  p.n_v = n_v;
  p.dim = dim;
  p.psi = dpsi.as<double>();
  p.inv_psi1 = dip.as<double>();
  p.a = o->a.as<double>();
  p.r = o->r.as<double>();
  p.b = o->b.as<double>();
  Check(launch_plda_dense_prep(p, nullptr), "dense PLDA preparation kernel launch");
  Check(hipDeviceSynchronize(), "dense PLDA preparation");   // the inputs are freed on return
}

// Rows [row0, row0 + m) of the score matrix into `out` (m x cols).
void ScoreChunk(const DenseOperands& o, int64_t row0, int m, double* out) {
  DenseGemmArgs g;
  g.p = (o.rows_are_v ? o.b : o.a).as<double>();
  g.q = (o.rows_are_v ? o.a : o.b).as<double>();
  g.row_add = o.rows_are_v ? nullptr : o.r.as<double>();
  g.col_add = o.rows_are_v ? o.r.as<double>() : nullptr;
  g.row0 = row0;
  g.m = m;
  g.n = o.cols();
  g.k_stride = o.ks;
  g.out = out;
  Check(launch_plda_dense_gemm(g, nullptr), "dense PLDA scoring kernel launch");
}

DensePlan PlanOrThrow(int64_t rows, int64_t cols, int dim) {
  DensePlan plan;
  std::string why;
  if (!PlanPldaDense(rows, cols, dim, DenseWorkspaceCap(), &plan, &why)) throw EngineError(why);
  return plan;
}

void CheckCounts(const char* who, const double* num_u, int n_u) {
  for (int k = 0; k < n_u; ++k)
    if (!(num_u[k] > 0)) throw EngineError(std::string(who) + ": example counts must be positive");
}

}  // namespace

int64_t DenseWorkspaceCap() {
  const char* e = getenv("XVEC_PLDA_DENSE_WORKSPACE");
  if (e && *e) {
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && !*end && v > 0) return (int64_t)v;
  }
  return kDenseDefaultWorkspace;
}

bool PlanPldaDense(int64_t rows, int64_t cols, int dim, int64_t workspace_bytes, DensePlan* out, std::string* why) {
  auto refuse = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (rows < 0 || cols < 1 || dim < 1 || workspace_bytes < 1) return refuse("dense PLDA plan: bad argument");
  if (dim > kPldaMaxDim) return refuse("dense PLDA plan: dimension larger than " + std::to_string(kPldaMaxDim));
  if (rows > 0x7fffffffll || cols > 0x7fffffffll) return refuse("dense PLDA plan: more than 2^31 - 1 rows or columns");
  int64_t rpc = workspace_bytes / (cols * 8);
  if (rpc < 1)
    return refuse("dense PLDA plan: a workspace of " + std::to_string(workspace_bytes) + " bytes does not hold one row of " +
                  std::to_string(cols) + " scores");
  if (rpc >= kDenseTileM) rpc -= rpc % kDenseTileM;                 // whole workgroup tiles
  rpc = std::min<int64_t>(rpc, (int64_t)65535 * kDenseTileM);       // the launch's grid
  out->rows_per_chunk = rpc;
  out->n_chunks = (rows + rpc - 1) / rpc;
  out->chunk_bytes = std::min(rows, rpc) * cols * 8;
  return true;
}

void PldaScoreDense(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim, const double* psi,
                    double* scores, float* device_ms) {
  if (n_u < 0 || n_v < 0 || dim < 1) throw EngineError("PldaScoreDense: bad shape");
  CheckDim(dim);
  CheckCounts("PldaScoreDense", num_u, n_u);
  UseDevice(device, kWhoNeeds);
  if (device_ms) *device_ms = 0.f;
  if (n_u == 0 || n_v == 0) return;
  const DensePlan plan = PlanOrThrow(n_u, n_v, dim);
  DenseOperands o;
  Prepare(u, num_u, n_u, v, n_v, dim, psi, false, &o);
  DevBuf chunk((size_t)plan.chunk_bytes);
  EventTimer tm(device_ms != nullptr);
  for (int64_t c = 0; c < plan.n_chunks; ++c) {
    const int64_t row0 = c * plan.rows_per_chunk;
    const int m = (int)std::min<int64_t>(plan.rows_per_chunk, n_u - row0);
    tm.Start();
    ScoreChunk(o, row0, m, chunk.as<double>());
    if (device_ms) *device_ms += tm.Stop();
    chunk.Download(scores + (size_t)row0 * n_v, (size_t)m * n_v * 8, "copy scores");
  }
}

void TopnStats(int device, const double* scores, int64_t rows, int cols, int n, double* mean, double* std, float* device_ms) {
  if (rows < 0 || rows > 0x7fffffffll || cols < 2 || cols > kTopnMaxCols || n < 2 || n > cols)
    throw EngineError("TopnStats: bad shape");
  UseDevice(device, kWhoNeeds);
  if (device_ms) *device_ms = 0.f;
  if (rows == 0) return;
  DevBuf dx((size_t)rows * cols * 8), dmean((size_t)rows * 8), dstd((size_t)rows * 8);
  dx.Upload(scores, (size_t)rows * cols * 8, "copy scores");
  TopnArgs t;
  t.x = dx.as<double>();
  t.rows = rows;
  t.cols = cols;
  t.n = n;
  t.mean = dmean.as<double>();
  t.std = dstd.as<double>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_topn_stats(t, nullptr), "top-N statistics kernel launch");
  if (device_ms) *device_ms = tm.Stop();
  dmean.Download(mean, (size_t)rows * 8, "copy means");
  dstd.Download(std, (size_t)rows * 8, "copy standard deviations");
}

void PldaCohortStats(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim, const double* psi,
                     bool by_column, int n, double* mean, double* std, float* device_ms) {
  if (n_u < 0 || n_v < 0 || dim < 1) throw EngineError("PldaCohortStats: bad shape");
  CheckDim(dim);
  const int64_t rows = by_column ? n_v : n_u;
  const int cols = by_column ? n_u : n_v;
  if (cols < 2 || cols > kTopnMaxCols || n < 2 || n > cols) throw EngineError("PldaCohortStats: bad shape");
  CheckCounts("PldaCohortStats", num_u, n_u);
  UseDevice(device, kWhoNeeds);
  if (device_ms) *device_ms = 0.f;
  if (rows == 0) return;
  const DensePlan plan = PlanOrThrow(rows, cols, dim);
  DenseOperands o;
  Prepare(u, num_u, n_u, v, n_v, dim, psi, by_column, &o);
  DevBuf chunk((size_t)plan.chunk_bytes), dmean((size_t)rows * 8), dstd((size_t)rows * 8);
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  for (int64_t c = 0; c < plan.n_chunks; ++c) {
    const int64_t row0 = c * plan.rows_per_chunk;
    const int m = (int)std::min<int64_t>(plan.rows_per_chunk, rows - row0);
    ScoreChunk(o, row0, m, chunk.as<double>());
    TopnArgs t;
    t.x = chunk.as<double>();
    t.rows = m;
    t.cols = cols;
    t.n = n;
    t.mean = dmean.as<double>() + row0;
    t.std = dstd.as<double>() + row0;
    Check(launch_topn_stats(t, nullptr), "top-N statistics kernel launch");   // stream order: before the next chunk is written
  }
  if (device_ms) *device_ms = tm.Stop();
  dmean.Download(mean, (size_t)rows * 8, "copy means");
  dstd.Download(std, (size_t)rows * 8, "copy standard deviations");
}

}  // namespace xv
